/* mvae.h -- C ABI of libmvae_hip.so: the MI355X (gfx950) kernels behind the SMILES-VAE training hot path.
 *
 * The reference (aclyde11/molecular-VAE) has no FFI or plugin layer: its hot path is the Python nn.Module
 * surface of models.py / mosesvae.py and the loop body of train.py:94-104, and all arithmetic is delegated
 * to torch.nn primitives.  This header is therefore the boundary the build defines *beneath* that surface
 * (SURVEY.md section 8b): one entry point per fused op x {fwd,bwd}; each comment names the reference call
 * site (file:line in the reference) whose torch primitive it replaces.
 *
 * Conventions
 *  - raw DEVICE pointers, caller-owned (the library never allocates or frees caller memory);
 *  - an explicit stream (hipStream_t passed as void*); every call is asynchronous on it and graph-capturable
 *    (no allocation, no synchronisation inside);
 *  - returns 0 on success, a negative MVAE_ERR_* for bad arguments, a positive hipError_t otherwise;
 *    never throws, never aborts;
 *  - no hidden RNG: noise (eps) is an input pointer;
 *  - matrices are row-major with explicit leading dimensions (in elements).  GEMM operands are read in
 *    16-byte chunks along K: K-extents that are not a multiple of the chunk (4 f32 / 8 bf16) require the
 *    rows to be zero-padded up to the next chunk boundary (the library's own producers do this);
 *  - dtype codes select the storage type of activations/weights inside the recurrent and GEMM kernels;
 *    accumulation, cell state, reductions, loss and optimiser state are always fp32.
 */
#ifndef MVAE_H_
#define MVAE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVAE_ABI_VERSION 12

#define MVAE_OK 0
#define MVAE_ERR_INVALID (-1)     /* bad argument (null pointer, bad size, misaligned leading dimension) */
#define MVAE_ERR_WORKSPACE (-2)   /* workspace too small */
#define MVAE_ERR_UNSUPPORTED (-3) /* combination not implemented */

#define MVAE_F32 0
#define MVAE_BF16 1
#define MVAE_F32X3 2   /* mvae_gemm_nt only: fp32 operands in memory, products on the bf16 MFMA as hi.hi + hi.lo + lo.hi (x = hi + lo in bf16):
                        ~16 mantissa bits per product, fp32 accumulation; shapes the LDS-direct loop does not serve run in exact fp32 */

#define MVAE_ACT_NONE 0
#define MVAE_ACT_SELU 1           /* models.py:58-68 */
#define MVAE_ACT_RELU 2           /* mosesvae.py:66-67 */

#define MVAE_CELL_LSTM 0          /* torch.nn.LSTM, gate rows [i;f;g;o]  (models.py:117,156) */
#define MVAE_CELL_GRU 1           /* torch.nn.GRU,  gate rows [r;z;n]    (mosesvae.py:54-61,73-79) */

#define MVAE_MAX_LAYERS 8

int mvae_abi_version(void);
/* sizeof of the descriptor structs as THIS library was compiled (0: mvae_rnn_fwd_desc, 1: mvae_rnn_bwd_desc, 2: mvae_gemm_tn_problem, 3: mvae_pack_job, 4: mvae_gemm_tn_f32_problem;
 * anything else: 0) -- a binding checks its own mirror of the structs against it at load time. */
size_t mvae_struct_size(int which);
const char* mvae_status_string(int status);
/* Schedule knobs (MVAE_BM, MVAE_BWD_SPLIT, ... : tile / split choices, every setting computes the same results) are read from the environment
 * ONLY while MVAE_TUNING=1 is set too; otherwise stray MVAE_* variables are ignored.  Returns the integer value of knob `name` as the library
 * would read it now, or `dflt`. */
int mvae_knob_int(const char* name, int dflt);

/* ---------------------------------------------------------------------------------------------------------
 * Dense contraction  C[M,N] = act( A[M,K] . B[N,K]^T + bias[N] )          (MFMA, fp32 accumulate)
 * Replaces nn.Linear at models.py:122,87-88,153,157 and mosesvae.py:66-67,81-82, and is the GEMM under the
 * conv / weight-gradient ops below.  dtype_ab: storage of A and B; dtype_c: storage of C.
 * accumulate != 0: C += result (fp32 C only; with a bf16 C the call is refused, MVAE_ERR_INVALID, nothing written).  ws: scratch for
 * split-K partials (may be NULL when mvae_gemm_nt_workspace() returns 0).
 * Operand rows are read in whole 16-byte chunks (4 f32 / 8 bf16 elements): the elements K .. roundup(K, chunk) - 1 of every row of A and
 * of B are read and must hold ZERO (so lda, ldb >= roundup(K, chunk)); nothing beyond them is read.  lda / ldb need not be multiples of
 * 16 bytes (such operands take the register-staged main loop instead of the LDS-direct one).  K == 0 reads nothing of A and B: C = act(bias),
 * zeros without a bias; under accumulate C += bias or stays as it was.  Columns N .. ldc - 1 of C are never written.
 * MVAE_F32X3 is honoured only where its own kernel runs (K a multiple of 4 and >= 128, 16-byte aligned rows, operands below 2 GiB; 128 x 128,
 * 128 x 64 or 64 x 128 tile, the operands split into bf16 hi / lo once per workgroup, K split as for MVAE_F32); elsewhere -- and on the 128 x 32 tile that N <= 32 with
 * M >= 128 takes -- the result is the exact-fp32 one.
 */
size_t mvae_gemm_nt_workspace(int M, int N, int K, int dtype_ab);
int mvae_gemm_nt(int dtype_ab, int M, int N, int K, const void* A, int64_t lda, const void* B, int64_t ldb,
                 void* C, int64_t ldc, int dtype_c, const float* bias, int act, int accumulate,
                 void* ws, size_t ws_bytes, void* stream);

/* C[M,N] = act( A^T . B + bias[N] ) with A [K, lda] and B [K, ldb] both K-major (row = k): the weight-gradient contraction
 * dW = dG^T . X reading dG [T*B, 4H] and X [T*B, H] as the recurrent kernels wrote them (hardware-transposed LDS reads, no
 * transposed copies).  bf16 operands: lda, ldb multiples of 8.  f32 operands (exact v_mfma_f32_16x16x4_f32 kernel): lda, ldb
 * multiples of 4, 16-byte aligned bases, fp32 C, no bias / activation.  Rows k >= K are never read.  Replaces autograd's weight-gradient GEMMs of models.py:128,164,157.
 * bf16: the pad columns M .. lda - 1 / N .. ldb - 1 ARE read, but reach only accumulators outside the matrix, which are not stored: they may
 * hold anything, NaN included.  K == 0: C = act(bias) (zeros without one), or C unchanged under accumulate.  bf16 operands of 2 GiB and more
 * (K * ld * 2 bytes) are contracted in equal K-chunks, one launch each, accumulating onto C: fp32 C, no bias / activation there
 * (MVAE_ERR_UNSUPPORTED otherwise). */
size_t mvae_gemm_tn_workspace(int M, int N, int K, int dtype_ab);
int mvae_gemm_tn(int dtype_ab, int M, int N, int K, const void* A, int64_t lda, const void* B, int64_t ldb,
                 void* C, int64_t ldc, int dtype_c, const float* bias, int act, int accumulate,
                 void* ws, size_t ws_bytes, void* stream);

/* fp32 (exact) form with the bias gradient:  C[M,N] (+)= A^T . B  and  colsum_out[m] (+)= sum_k A[k][m]  from the same MFMAs -- B gets a virtual
 * column of ones at index N, in the slack of the last 64-wide tile (a whole extra tile column only when N % 64 == 0).  Replaces the
 * mvae_gemm_tn + mvae_colsum pair behind every nn.Linear / nn.LSTM bias of the fp32 encoder.  ws >= mvae_gemm_tn_workspace(MVAE_F32). */
int mvae_gemm_tn_f32_colsum(int M, int N, int K, const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int accumulate,
                            float* colsum_out, int colsum_accumulate, void* ws, size_t ws_bytes, void* stream);

/* bf16 weight gradient AND bias gradient from one pass over dG:  C[M,N] (+)= A^T . B  and  colsum_out[m] (+)= sum_k A[k][m].
 * The column sums come from ONE extra MFMA per wave and K-step (an A fragment against a fragment of ones) inside the 256 x 256-tile
 * kernel, shared out over the 16 waves that hold the same A rows, so they cost no extra HBM traffic (a separate mvae_colsum_t re-reads
 * all of dG).  Only for shapes that kernel serves with 4 tile columns and split-K (mvae_gemm_tn_colsum_supported: N == 1024, M >= 2048,
 * K >= 4096); otherwise MVAE_ERR_UNSUPPORTED.  fp32 C, no bias / activation. */
int mvae_gemm_tn_colsum_supported(int M, int N, int K);
/* Grouped form: up to 2 * MVAE_MAX_LAYERS contractions of that kind in ONE launch, each 256 x 256 output tile accumulated in registers over
 * its problem's full K -- no split-K slabs, no reduction launch (the decoder's 7 dW_ih / dW_hh GEMMs are 7 x 64 tiles >= 256 CUs).
 * colsum_out (optional, needs N == 1024) as above; ws >= mvae_gemm_tn_grouped_workspace bytes (two K-half column-sum partials per
 * problem that asks for them, summed in a fixed order by a tiny second launch).  Problems must pass mvae_gemm_tn_grouped_supported. */
typedef struct {
  int M, N; int64_t K;
  const void* A; int64_t lda;          /* [K, lda] bf16, K-major */
  const void* B; int64_t ldb;          /* [K, ldb] bf16 */
  float* C; int64_t ldc; int accumulate;
  float* colsum_out; int colsum_accumulate;
} mvae_gemm_tn_problem;
int mvae_gemm_tn_grouped_supported(int M, int N, int64_t K, int64_t lda, int64_t ldb);
size_t mvae_gemm_tn_grouped_workspace(int n, const mvae_gemm_tn_problem* problems);
int mvae_gemm_tn_grouped(int n, const mvae_gemm_tn_problem* problems, void* ws, size_t ws_bytes, void* stream);
/* The same launch with at most `max_workgroups` workgroups (0: one per tile), each looping over tiles: a throughput-bound group of GEMMs on a
 * side stream that must leave compute units to the latency-bound launches of the main stream (the per-rank batch of a data-parallel job:
 * K = T * b is short, the encoder's backward runs beside it). */
int mvae_gemm_tn_grouped_capped(int n, const mvae_gemm_tn_problem* problems, int max_workgroups, void* ws, size_t ws_bytes, void* stream);
/* Exact-f32 TN contractions of DIFFERENT shapes in ONE launch (+ one reduction launch for all of their split-K slabs): the parameter-gradient
 * GEMMs of the encoder's backward pass -- Lambda heads, dense_1, the three Conv1d weight gradients, the LSTM(72) stack's dW_ih / dW_hh
 * (models.py:87-88,122,118-120,117) -- are a dozen small dependent-free products whose only consumer is the optimiser; launched one by one
 * each leaves most of the chip idle.  Problem i: C[M,N] (+)= A^T . B over K rows, A / B row-major fp32 with optional row groups (row r starts
 * at (r / group) * gstride + (r % group) * ld when group > 0: the overlapping windows of a channels-last Conv1d), colsum_out (optional):
 * column sums of A through a virtual ones column (as mvae_gemm_tn_f32_colsum), x3 != 0: products as 3 x bf16 (MVAE_F32X3).  lda, ldb and the
 * group strides multiples of 4, bases 16-byte aligned.  At most MVAE_TN_F32_MULTI_MAX problems; outputs must not overlap.  Every problem needs
 * M >= 1 and N >= 1 (K == 0 is served: C = 0 or unchanged): n outside 1 .. MVAE_TN_F32_MULTI_MAX or an empty problem is MVAE_ERR_INVALID for
 * the whole call, with nothing launched. */
#define MVAE_TN_F32_MULTI_MAX 16
typedef struct {
  int M, N; int64_t K;
  const float* A; int64_t lda; int a_group; int64_t a_gstride;
  const float* B; int64_t ldb; int b_group; int64_t b_gstride;
  float* C; int64_t ldc; int accumulate;
  float* colsum_out; int colsum_accumulate;
  int x3;
} mvae_gemm_tn_f32_problem;
size_t mvae_gemm_tn_f32_multi_workspace(int n, const mvae_gemm_tn_f32_problem* problems);
int mvae_gemm_tn_f32_multi(int n, const mvae_gemm_tn_f32_problem* problems, void* ws, size_t ws_bytes, void* stream);
size_t mvae_gemm_tn_colsum_workspace(int M, int N, int K);
int mvae_gemm_tn_colsum(int M, int N, int K, const void* A, int64_t lda, const void* B, int64_t ldb, float* C, int64_t ldc, int accumulate,
                        float* colsum_out, int colsum_accumulate, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Data movement helpers.
 */
/* dst[r, c] = (Td) src[r, c] for r<R, c<C; columns C..ldd-1 of dst are zeroed.  When dstT != NULL also
 * dstT[c, r] = (Td) src[r, c] with columns R..ldt-1 zeroed.  Weight packing (fp32 master -> bf16 shadow and
 * its transpose) and activation transposes. */
int mvae_cast_transpose(int dtype_src, int dtype_dst, int R, int C, const void* src, int64_t lds_,
                        void* dst, int64_t ldd, void* dstT, int64_t ldt, void* stream);

/* Multi-tensor pack: a LIST of small packing jobs in one launch (a model refreshes dozens of weight shadows after every optimiser step:
 * fp32 master -> bf16 / zero-padded / transposed copies, bias sums, block copies -- each a few-microsecond launch of its own otherwise).
 *   kind 0: dst[r, c] and / or dstT[c, r] = (dst_dtype) src[r, c] for r < R, c < C only (no zero fill of padding: allocate destinations zeroed);
 *   kind 1: dst[i] = src[i] + src2[i], fp32, R * C elements (b_ih + b_hh);   kind 2: dst[r, c] = src[r, c], fp32, leading dimensions lds / ldd.
 * `jobs_device` is an array in DEVICE memory (build it once: the pointers do not change from step to step); block0 = index of the job's
 * first block = sum of mvae_pack_job_blocks() of the jobs before it; total_blocks = the sum over all jobs.  Jobs must not overlap. */
typedef struct {
  int kind, src_dtype, dst_dtype, R, C, block0;
  const void* src; int64_t lds;
  void* dst; int64_t ldd;
  void* dstT; int64_t ldt;
  const void* src2;
} mvae_pack_job;
int mvae_pack_job_blocks(const mvae_pack_job* job);
int mvae_pack_multi(int njobs, const mvae_pack_job* jobs_device, int total_blocks, void* stream);

/* out[n, b, a] = in[n, a, b] (fp32): the channel-major Flatten of models.py:6-10 <-> the conv GEMM's row order. */
int mvae_permute021(int N, int A, int Bd, const float* in, float* out, void* stream);

/* out[(t*B + b), :] = table[idx[b*L + t], :]   (fp32, W columns).  models.py:127 nn.Embedding, fused with the
 * layer-0 input projection: table = E . W_ih0^T + b. */
int mvae_gather_rows_tb(const int64_t* idx, int B, int L, int nrows, const float* table, int W, const float* base /* optional [B, W] per-sequence addend */,
                        float* out, void* stream);
/* dtable[c, :] = sum over (t,b) with idx[b*L+t]==c of d[(t*B+b), :]   (deterministic).  d has dtype `dtype`. */
int mvae_scatter_rows_tb(int dtype, const int64_t* idx, int B, int L, int nrows, const void* d, int64_t ldd, int W,
                         float* dtable, void* ws, size_t ws_bytes, void* stream);
size_t mvae_scatter_rows_tb_workspace(int B, int L, int nrows, int W);
/* out[(t*B + b), c] = (idx[b*L + t] == c) ? 1 : 0  for c < ld (bf16 [L*B, ld], ld >= nrows, ld % 8 == 0; ids clamped as in the gather).
 * With it the scatter above is the TN contraction  dtable = out^T . d  (mvae_gemm_tn, M = nrows): the bf16 gradient sequence is read
 * once at GEMM streaming rate and summed in fp32 by the MFMAs. */
int mvae_onehot_tb(const int64_t* idx, int B, int L, int nrows, void* out, int64_t ld, void* stream);
/* fp32 form, rows in the order of idx itself: out[r, c] = (idx[r] == c) for r < n, c < ld (ld >= nrows, ld % 4 == 0; ids clamped to
 * [0, nrows) as in the gather).  The exact-f32 table gradient
 * of the encoder (models.py:116 Embedding folded into the LSTM's layer-0 projection) is then one problem of mvae_gemm_tn_f32_multi: A = out,
 * B = the layer-0 pre-activation gradients addressed through row groups (row b * L + t of B = dG[t][b]). */
int mvae_onehot_f32(const int64_t* idx, int64_t n, int nrows, float* out, int64_t ld, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Recurrent stack (K2, K7, K10, K12 of SURVEY.md): torch.nn.LSTM / nn.GRU, batch-major module semantics,
 * zero (LSTM) or given (GRU) initial state, time-major storage here.  Replaces models.py:128, models.py:164,
 * mosesvae.py:153, mosesvae.py:188.
 *
 * Schedule: layer-wavefront.  Launch d updates every cell (layer l, time t = d - l); one launch computes, for
 * up to `layers` cells,   pre = x_t . W_ih^T + h_{t-1} . W_hh^T + bias   (two K-segments of one MFMA tile
 * loop) and applies the gate non-linearities and the state update in the epilogue.
 *
 * Layer 0 input is either a real sequence x0 [T*B, in0] (dtype) or a precomputed fp32 pre-activation
 * addend add0 (row (t*B+b) at add0 + t*add0_tstride + b*G*H; tstride 0 = time-invariant input, models.py:163
 * Repeat), or both.  A token input that was folded into W_ih (embedding . W_ih^T = a [rows, G*H] fp32 table, mosesvae.py:150-153,
 * 176-188) is given as add_table + add_index: cell (0, t) adds table row add_index[b * add_index_ld + t] to row b in its epilogue,
 * on top of add0 -- the gathered [T, B, G*H] sequence is never written.  bias[l] (fp32 [G*H]) is added for layers whose input is a
 * real sequence.
 *
 * Saved for backward (all caller-allocated):
 *   hs[l]     [T][B][ldh]   dtype   layer outputs h_t          (hs[layers-1] is the stack output)
 *   cs[l]     [T][B][H]     dtype   cell states as the backward pass reads them (LSTM only)
 *   gates[l]  [T][B][G*H]   dtype   post-activation gates i,f,g,o (LSTM) / r,z,n,(W_hn h + b_hn) (GRU)
 *   A forward-only call (evaluation under no_grad, train.py:120-153) passes gates[l] == cs[l] == NULL for EVERY layer: the
 *   kernels then skip the saved-state stores (12 of the 16 bytes written per (row, unit, step)); hs / cstate are still written.
 *   cstate[l] [2][B][H]     fp32    scratch: the recurrent cell state itself stays fp32 (ping-pong over t)
 * lengths (GRU path): per-sequence valid length, sorted descending (pack_sequence semantics: a finished
 * sequence keeps its last state and emits zeros); NULL = all T.
 */
typedef struct {
  int cell, dtype, layers, T, B, H, in0;
  const void* x0; int64_t x0_ld;
  const float* add0; int64_t add0_tstride;
  const float* add_table; const int64_t* add_index; int64_t add_index_ld; int add_table_rows;   /* optional (NULL): see above; ids are clamped to the table */
  const void* w_ih[MVAE_MAX_LAYERS]; int64_t ldw_ih[MVAE_MAX_LAYERS];   /* [G*H, in] (w_ih[0] unused when x0 == NULL) */
  const void* w_hh[MVAE_MAX_LAYERS]; int64_t ldw_hh[MVAE_MAX_LAYERS];   /* [G*H, H] */
  const float* bias[MVAE_MAX_LAYERS];                                    /* LSTM: b_ih+b_hh [4H]; GRU: [b_ir+b_hr; b_iz+b_hz; b_in; b_hn] [4H] */
  const void* h0[MVAE_MAX_LAYERS]; int64_t ldh0;                         /* GRU: optional initial hidden state [B, ldh0] dtype (NULL = zeros).  LSTM: must be NULL
                                                                            (zero initial state, there is no c0): any h0[l] != NULL -> MVAE_ERR_UNSUPPORTED */
  const int32_t* lengths;
  void* hs[MVAE_MAX_LAYERS]; int64_t ldh;
  void* cs[MVAE_MAX_LAYERS];
  void* gates[MVAE_MAX_LAYERS];
  float* cstate[MVAE_MAX_LAYERS];
  int zero_padded_k;   /* != 0: rows of hs, h0, w_ih (l>0) and w_hh are allocated AND zero up to the next multiple of 128 bytes
                          past H, so the contraction may run over whole K-steps (enables the LDS-direct main loop for e.g. H = 72) */
  /* Inter-layer dropout (torch.nn.GRU(dropout=p), train mode; mosesvae.py:73-79): layer l+1 reads  hdrop[l] = hs[l] * keep / (1 - p)
   * instead of hs[l] (the recurrence of layer l itself still reads hs[l]).  hdrop[l] [T][B][ldh] dtype for l < layers-1, all NULL = no
   * dropout.  keep(l,t,b,j) comes from drop_mask[l] ([T][B][H] bytes, 1 = keep) when given (parity tests inject the reference's draw),
   * else from the counter-based hash  mvae_dropout_keep(drop_seed, ((l*T + t)*B + b)*H + j, drop_p)  -- no hidden RNG state. */
  void* hdrop[MVAE_MAX_LAYERS];
  const uint8_t* drop_mask[MVAE_MAX_LAYERS];
  float drop_p; uint32_t drop_seed;
  /* Optional second schedule, the WEIGHTS-RESIDENT DATAFLOW pass (rnn_persist.hip): ONE persistent launch of 256 workgroups in which every
   * workgroup keeps its 256 KB slice of [W_ih | W_hh] in registers for all T steps and the h_t tiles travel between workgroups through
   * write-through stores + flag words (no launch per diagonal).  Serves the per-rank shape of the 8-GPU configuration only (LSTM, bf16,
   * 4 layers, H = 1024, B = 128, zero initial state, time-invariant layer-0 input, ldh = H + 64, a 256-CU device with nothing else running
   * beside it): mvae_rnn_fwd_persist_workspace() returns 0 for everything else.  persist_ws != NULL (that many bytes of device memory,
   * 16-byte aligned) selects it; the first 16 bytes are a status record the launch leaves behind -- word 0 != 0: a bounded spin ran out
   * (a workgroup was not resident, or a producer died), the outputs are invalid; the launch itself always ends.
   * The narrow exact-f32 stacks (LSTM, H = 72: the encoder, models.py:117,128) use the same scratch for their LAYER-CONCURRENT row-resident form
   * (rnn_rowres.hip: all layers in one launch as a pipeline over per-workgroup progress words, when layers x ceil(B / 4) workgroups are resident
   * at once); same status convention.
   * poison (optional, device fp32 word): a launch of this call that gives up ALSO stores a quiet NaN there -- the caller points it at the
   * spare slot behind its flat gradient buffer, so that mvae_sumsq / mvae_clip_adam skip the whole update of a step whose forward or
   * backward pass produced garbage (and, in data parallel, every rank skips it: the slot travels with the gradient all-reduce).  Nothing
   * is ever written there by a launch that succeeds. */
  void* persist_ws; size_t persist_ws_bytes;
  float* poison;
  int no_spin;         /* != 0: never take a schedule that contains bounded spins (the caller's fallback after a launch that gave up) */
} mvae_rnn_fwd_desc;

/* keep decision of the device-generated dropout mask (host-callable restatement: the oracle and the tests use the same hash):
 *   h = idx * 0x9E3779B1 ^ seed; h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16;  keep = h >= (uint32)(p * 2^32) */
int mvae_dropout_keep(uint32_t seed, uint32_t idx, float p);

/* status_out (optional): receives the device address of the 16-byte status record the launches THIS call enqueued will leave behind (word 0
 * != 0: a bounded spin ran out, the outputs are invalid; words 1-2: who), or NULL when the schedule it took contains no bounded spin (the
 * wavefront and layer-by-layer schedules: nothing to check).  The library, not the caller, knows which schedule ran. */
int mvae_rnn_fwd(const mvae_rnn_fwd_desc* d, void* stream, const void** status_out);
size_t mvae_rnn_fwd_persist_workspace(const mvae_rnn_fwd_desc* d);   /* 0: this shape / device is not served by the persistent schedule */

/* Backward through time of the same stack (reverse wavefront).  One launch computes, per cell,
 *   dh_t = dG^{l}_{t+1} . W_hh + dG^{l+1}_t . W_ih^{l+1} (+ dy_t for the top layer)
 * and, in the epilogue, the gate derivative dG^{l}_t (pre-activation gradient) and dc_{t-1}.
 *   w_hhT[l] [H, G*H], w_ihT[l] [in, G*H]: TRANSPOSED weights (K-contiguous for this contraction).
 *   dy       [T][B][H] fp32 gradient w.r.t. the stack output (row stride dy_ld).
 *   dy_a / dy_w / dy_k (optional, dtype bf16; GRU: rows of finished sequences must be zero in dy_a): the same gradient given as a product  dy_t = dy_a[t] . dy_w^T  with
 *            dy_a [T][B][dy_a_ld] dtype (e.g. the logit gradients of TimeDistributed(Linear), models.py:157) and dy_w [H][dy_w_ld] dtype
 *            (the Linear's weight, transposed), both zero-padded to dy_k columns, dy_k a multiple of 128: the TOP layer's cell contracts it
 *            as its second K-segment (that cell has no layer above), so the [T, B, H] fp32 tensor is never written or read.
 *            dy and dy_a may both be given (they add).
 *   dG[l]    [T][B][ldg]  dtype  (out)  pre-activation gradients (G*H valid columns); dG[0] is also the gradient of add0.
 *   dstate[l] [2][B][H] fp32 scratch (ping-pong dc).
 * Weight / bias / input gradients are then mvae_gemm_tn(dG[l], hs[l-1] / hs[l] shifted by one step) and mvae_colsum_t(dG[l]).
 */
typedef struct {
  int cell, dtype, layers, T, B, H;
  const void* w_hhT[MVAE_MAX_LAYERS]; int64_t ldw_hhT[MVAE_MAX_LAYERS];
  const void* w_ihT[MVAE_MAX_LAYERS]; int64_t ldw_ihT[MVAE_MAX_LAYERS];   /* w_ihT[0] unused */
  const int32_t* lengths;
  const float* dy; int64_t dy_ld;
  const void* dy_a; int64_t dy_a_ld; const void* dy_w; int64_t dy_w_ld; int dy_k;   /* optional (NULL): see above */
  const float* dh_last[MVAE_MAX_LAYERS];                                  /* GRU: optional fp32 [B,H] gradient w.r.t. the final hidden state.  LSTM: must be NULL */
  const void* hs[MVAE_MAX_LAYERS]; int64_t ldh;
  const void* h0[MVAE_MAX_LAYERS]; int64_t ldh0;                          /* GRU only, as in mvae_rnn_fwd_desc.  LSTM: h0[l], dh_last[l] and dh0[l] must all be
                                                                             NULL -- a non-NULL one is refused with MVAE_ERR_UNSUPPORTED before anything is enqueued */
  const void* cs[MVAE_MAX_LAYERS];
  const void* gates[MVAE_MAX_LAYERS];
  void* dG[MVAE_MAX_LAYERS]; int64_t ldg;                                  /* row stride of dG (>= G*H; pad it off powers of two) */
  void* dGh[MVAE_MAX_LAYERS];                                              /* RESERVED, ignored: no kernel reads or writes it (the W_hh-side rows are dG's slots r, z, n*r); kept for the struct layout */
  float* dstate[MVAE_MAX_LAYERS];                                         /* fp32 [2][B][H] ping-pong: LSTM dc, GRU dh carry */
  float* dh0[MVAE_MAX_LAYERS];                                            /* GRU: optional out: gradient w.r.t. h0 (decoder_lat path).  LSTM: must be NULL */
  void* split_ws; size_t split_ws_bytes;                                  /* optional scratch of mvae_rnn_bwd_workspace(d) bytes: enables the split-K
                                                                             schedules (fp32 partial tiles of dh summed across workgroups) */
  /* inter-layer dropout of the forward pass (same mask / seed / p): the gradient that layer l receives from layer l+1
   * (dG^{l+1}_t . W_ih^{l+1}) is multiplied by keep(l,t,b,j) / (1 - p).  drop_p == 0: no dropout. */
  const uint8_t* drop_mask[MVAE_MAX_LAYERS];
  float drop_p; uint32_t drop_seed;
  /* Optional second schedule, the WEIGHTS-RESIDENT DATAFLOW backward (rnn_persist_bwd.hip), the counterpart of mvae_rnn_fwd_desc.persist_ws: ONE
   * persistent launch of 256 workgroups, each keeping a (64 hidden units x one gate's K-quarter) slice of [W_hh^T | W_ih^T] in registers for
   * all T steps; the dG tiles and the K-quarter partial sums travel between workgroups through write-through stores + flag words.  Serves
   * LSTM, bf16, 4 layers, H = 1024, B = 128 (256: two passes), ldg = 4H + 64, the output gradient given as dy (fp32, dy_ld = H; not dy_a), no
   * dh_last / dropout, on a 256-CU device with nothing else running beside it: mvae_rnn_bwd_persist_workspace() returns 0 for everything else.
   * persist_ws != NULL (that many bytes, 16-byte aligned) selects it; its first 16 bytes are the status record (word 0 != 0: a bounded spin
   * ran out, dG is invalid).  dstate is not written by this schedule (the carried dc never leaves the registers).
   * poison: as in mvae_rnn_fwd_desc (also honoured by the layer-concurrent row-resident backward, whose status record lives inside split_ws). */
  void* persist_ws; size_t persist_ws_bytes;
  float* poison;
  int no_spin;         /* as in mvae_rnn_fwd_desc */
} mvae_rnn_bwd_desc;

int mvae_rnn_bwd(const mvae_rnn_bwd_desc* d, void* stream, const void** status_out);     /* status_out: see mvae_rnn_fwd */
size_t mvae_rnn_bwd_persist_workspace(const mvae_rnn_bwd_desc* d);   /* 0: this shape / device is not served by the persistent schedule */
/* bytes of split_ws that let mvae_rnn_bwd pick any of its schedules for this shape (reads layers, T, B, H only). */
size_t mvae_rnn_bwd_workspace(const mvae_rnn_bwd_desc* d);

/* out[r] = sum_c X[r, c]  (X dtype, fp32 out; one wave per row, fixed order): bias gradients from dGT. */
int mvae_rowsum(int dtype, int R, int C, const void* X, int64_t ldx, float* out, int accumulate, void* stream);
/* out[b, :] = sum_t X[t, b, :]  (fp32 out): gradient of a time-invariant layer-0 input (models.py:163). */
int mvae_timesum(int dtype, int T, int B, int W, const void* X, float* out, void* stream);
/* out[n] = sum_m X[m, n] (fp32 in/out, deterministic two-stage): bias gradients of the dense / conv layers. */
size_t mvae_colsum_workspace(int M, int N);
int mvae_colsum(int M, int N, const float* X, int64_t ldx, float* out, void* ws, size_t ws_bytes, void* stream);
/* same for X of `dtype` read in 16-byte vectors (ldx multiple of 8, X 16-byte aligned): bias gradients from dG [T*B, G*H]. */
size_t mvae_colsum_t_workspace(int M, int N);
int mvae_colsum_t(int dtype, int M, int N, const void* X, int64_t ldx, float* out, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Conv1d(k) + bias + SELU, valid, stride 1 (K3; models.py:71-77 ConvSELU, :118-120, :129-131) as a
 * sliding-window MFMA GEMM (exact f32).  Activations are CHANNELS-LAST with padded channel count:
 *   x[b, w, c] = x[b * x_bs + w * ldx + c],  c < Cin valid, channels [Cin, ldx) must be zero;
 *   y[b, w, o] = y[(b * Wout + w) * ldy + o], Wout = W - k + 1 (columns [Cout, ldy) are not written).
 * The im2col row of (b, w) is the contiguous range x[b, w : w+k, :], so no im2col matrix exists; weights are
 * repacked per step by mvae_conv1d_pack_weights:
 *   wp [Cout][k * ldx]: wp[o][j * ldx + c] = w[o][c][j]          (forward / weight gradient; pads zero)
 *   wq [Cin][k * ldo] : wq[c][j * ldo + o] = w[o][c][k - 1 - j]  (input gradient; pads zero)      either may be NULL.
 * The LDS-direct main loop needs k * ldx (forward) / k * ldo (input gradient) to be a multiple of 32; other
 * sizes run on the generic loop.
 */
int mvae_conv1d_pack_weights(int Cin, int Cout, int k, const float* w /* [Cout, Cin, k] */, int ldx, float* wp, int ldo, float* wq,
                             void* stream);
size_t mvae_conv1d_selu_fwd_workspace(int B, int W, int ldx, int Cout, int k);
int mvae_conv1d_selu_fwd(int B, int W, int ldx, int64_t x_bs, int Cout, int k, const float* x, const float* wp, const float* bias,
                         float* y, int64_t ldy, void* ws, size_t ws_bytes, void* stream);
/* dy, y: [B * Wout, ldo] (gradient w.r.t. y / forward output; ldo % 4 == 0), x: the forward input (ldx % 4 == 0, x_bs % 4 == 0).
 * dzp: scratch [B, Wout + 2(k-1), ldo] -- receives the zero-padded pre-activation gradient.
 * dw [Cout, Cin, k] and db [Cout] in the reference's parameter layout; dx [B * W, lddx] channels-last (NULL: not needed; else wq required).
 * All pointers 16-byte aligned.  ws: scratch >= mvae_conv1d_selu_bwd_workspace bytes. */
size_t mvae_conv1d_selu_bwd_workspace(int B, int W, int Cin, int ldx, int Cout, int ldo, int k);
/* The same pair with the activation as a parameter (MVAE_ACT_NONE / _SELU / _RELU; same workspaces): Conv1d + ReLU of the
 * models2d.VAE encoder (models2d.py:12-14,24-27). */
int mvae_conv1d_act_fwd(int act, int B, int W, int ldx, int64_t x_bs, int Cout, int k, const float* x, const float* wp, const float* bias,
                        float* y, int64_t ldy, void* ws, size_t ws_bytes, void* stream);
/* OR-ed into `act` of mvae_conv1d_act_bwd: the input-gradient AND weight-gradient GEMMs multiply in the MVAE_F32X3 form (gradients only: the bf16 training mode,
 * whose decoder gradients are bf16-accurate anyway; the forward conv and the exact-fp32 mode never use it). */
#define MVAE_CONV_BWD_X3 0x100
int mvae_conv1d_act_bwd(int act, int B, int W, int Cin, int ldx, int64_t x_bs, int Cout, int ldo, int k, const float* dy, const float* y,
                        const float* x, const float* wq, float* dzp, float* dw, float* db, float* dx, int64_t lddx,
                        void* ws, size_t ws_bytes, void* stream);
/* dw == NULL in mvae_conv1d_*_bwd: only dzp and dx are produced; the layer's weight / bias gradient is then described by mvae_conv1d_dw_problem
 * as one problem of mvae_gemm_tn_f32_multi (dwp [Cout][k * ldx]: the gradient in the packed layout of wp; db: bias gradient) and brought into
 * the parameter layout dw [Cout][Cin][k] by mvae_conv1d_unpack_dw -- so that ALL parameter gradients of an encoder share one launch. */
int mvae_conv1d_dw_problem(int B, int W, int Cin, int ldx, int64_t x_bs, int Cout, int ldo, int k, const float* dzp, const float* x, float* dwp,
                           float* db, int x3, mvae_gemm_tn_f32_problem* out);
int mvae_conv1d_unpack_dw(int Cin, int Cout, int k, const float* dwp, int ldx, float* dw, void* stream);
int mvae_conv1d_selu_bwd(int B, int W, int Cin, int ldx, int64_t x_bs, int Cout, int ldo, int k, const float* dy, const float* y,
                         const float* x, const float* wq, float* dzp, float* dw, float* db, float* dx, int64_t lddx,
                         void* ws, size_t ws_bytes, void* stream);

/* dpre = dy * SELU'(pre) expressed through the forward OUTPUT y (in place on dy).  models.py:58-68. */
int mvae_selu_bwd(int64_t n, float* dy, const float* y, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Lambda / reparameterisation (K5; models.py:80-94).  mulv [B, 2*o]: mu | log_var (one stacked GEMM).
 * z = mu + exp(log_var/2) * eps        eps [B,o] is the already scaled noise (reference: 1e-2 * randn).
 * Noise source (models.py:92 draws it on the CPU default generator; SURVEY 8b: "eps|null, seed"):
 *   eps != NULL  the caller's noise is used as it is (parity tests, the reference's CPU RNG stream); scale / seed / offset ignored.  The pointer
 *                may be device memory or device-mapped PINNED HOST memory (hipHostMalloc / torch pin_memory), which the launch reads in place --
 *                no copy command in the stream; eps_out (optional) then receives a device copy for the backward pass;
 *   eps == NULL  the draw happens INSIDE this launch: element i of the [B, o] block is scale * n(seed, offset + i), n = a standard normal
 *                from the counter hash below (no generator state anywhere: the same (seed, offset) always yields the same block), and is
 *                written to eps_out [B, o] (required then), which is what mvae_lambda_bwd takes as eps.
 * Backward: dmulv[:, :o] = dmu + dz ; dmulv[:, o:] = dlogvar + dz * eps * 0.5 * exp(log_var/2).
 *
 * The counter normal n(seed, c), c a 64-bit element counter: s = H(seed, (c >> 31) ^ 0x6A09E667), w1 = H(s, 2c mod 2^32),
 * w2 = H(s ^ 0xBB67AE85, (2c mod 2^32) | 1) with H the counter hash of mvae_dropout_keep; u1 = ((w1 >> 8) + 0.5) / 2^24, u2 = (w2 >> 8) / 2^24,
 * n = sqrt(-2 ln u1) * cos(2 pi u2).  mvae_normal_words returns (w1, w2) computed on the HOST by the same function the kernels compile
 * (tests restate the draw from them); mvae_normal_fill writes out[i] = scale * n(seed, offset + i), i < n (mosesvae.py:159 / models2d.py:34
 * randn_like as a library op).
 */
int mvae_lambda_fwd(int B, int o, const float* mulv, const float* eps, float scale, uint32_t seed, uint64_t offset, float* eps_out,
                    float* z, float* mu, float* logvar, void* stream);
int mvae_normal_fill(int64_t n, float scale, uint32_t seed, uint64_t offset, float* out, void* stream);
void mvae_normal_words(uint32_t seed, uint64_t counter, uint32_t* words2);
int mvae_lambda_bwd(int B, int o, const float* mulv, const float* eps, const float* dz, const float* dmu,
                    const float* dlogvar, float* dmulv, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Output head (K8; models.py:157 Linear + nn.Softmax() over the class axis of the [B*L, C] view,
 * models.py:43-50).  logits [(t*B+b), ldl] fp32 -> recon [B, L, C] fp32 probabilities.
 * Backward: dlogits = p * (drecon - sum_c drecon*p), written in dtype as dl [(t*B+b), ldd] and, when dlT != NULL, transposed
 * dlT [C][ldT] (column t*B+b).  Columns C .. C8-1 (C8 = C rounded up to 8) of dl are written as zero; the K-padding columns C8 .. ldd-1
 * are the CALLER's to keep zero (allocate the buffer zeroed: this call may or may not touch them -- the tiled bf16 form does not).
 */
int mvae_softmax_tb_fwd(int B, int L, int C, const float* logits, int64_t ldl, float* recon, void* stream);
int mvae_softmax_tb_bwd(int dtype, int B, int L, int C, const float* recon, const float* drecon,
                        void* dl, int64_t ldd, void* dlT, int64_t ldT, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * ELBO of train.py:31-38, verbatim: max_len * BCELoss(mean)(recon, x) - 0.5*mean(1 + mu - logvar^2 - exp(mu))
 * (binary CE on the softmax outputs with the log clamp at -100; mu / logvar swapped in the KL term, as the
 * reference computes it).  loss_out[0] = total, [1] = xent term, [2] = KL term.  ONE launch: per-block partial sums, a ticket counter, and
 * the block drawing the last ticket sums the partials in a fixed order (deterministic).  ws >= mvae_bce_kl_loss_workspace() bytes, 4-byte
 * aligned, private to this call site; its LAST 16 BYTES (the ticket) must be zero before the first call -- every call leaves them zero again.
 * Backward: drecon = g*(max_len/n)*(p - t)/max(p(1-p),1e-12); dmu = g*(-0.5/m)(1 - exp(mu));
 * dlogvar = g*(0.5/m)*2*logvar, with g = *grad_out (device scalar) or 1 when NULL.
 */
size_t mvae_bce_kl_loss_workspace(int64_t n_recon, int64_t n_latent);
int mvae_bce_kl_loss_fwd(int64_t n_recon, const float* recon, const float* target, int64_t n_latent, const float* mu,
                         const float* logvar, float max_len, float* loss_out, void* ws, size_t ws_bytes, void* stream);
int mvae_bce_kl_loss_bwd(int64_t n_recon, const float* recon, const float* target, int64_t n_latent, const float* mu,
                         const float* logvar, float max_len, const float* grad_out, float* drecon, float* dmu,
                         float* dlogvar, void* stream);

/* The same ELBO from the head's TIME-MAJOR logits [(t*B+b), ldl] fp32 and the int64 index targets idx [B, L] (batch-major): the softmax over
 * C, the BCE against the implied one-hot (-log p_y - sum_{c != y} log(1 - p_c), each log clamped at -100), the mean over B*L*C times
 * max_len, and the KL term above -- without the [B, L, C] probabilities, the float one-hot or drecon.  C <= 128 (else MVAE_ERR_UNSUPPORTED);
 * n_latent = the element count of mu / logvar.
 *   fwd: loss_out[3] as mvae_bce_kl_loss_fwd (one launch, the same deterministic ticket reduction; ws >= mvae_bce_kl_logits_workspace()
 *   bytes with the same zero-ticket contract).  pred_out (optional) int64 [B, L]: the arg-max of each row's probabilities, first index on
 *   ties (recon.argmax(2)).  An index outside [0, C) is never dereferenced: it makes the loss NaN.
 *   bwd: dl = softmax_bwd(p, drecon) with drecon = g*(max_len/n)*(p - onehot)/max(p(1-p),1e-12), p recomputed from the logits, written in
 *   dtype to dl [(t*B+b), ldd] (columns C .. ldd-1 are not touched: the caller keeps them zero) and, when dlT != NULL, to dlT [C][ldT]
 *   (column t*B+b, ldT >= B*L); dmu / dlogvar of the KL term come from the same launch.  g = *grad_out, or 1 when NULL.
 */
size_t mvae_bce_kl_logits_workspace(int B, int L);
int mvae_bce_kl_logits_fwd(int B, int L, int C, const float* logits, int64_t ldl, const int64_t* idx, int64_t n_latent, const float* mu,
                           const float* logvar, float max_len, float* loss_out, int64_t* pred_out, void* ws, size_t ws_bytes, void* stream);
int mvae_bce_kl_logits_bwd(int dtype, int B, int L, int C, const float* logits, int64_t ldl, const int64_t* idx, int64_t n_latent,
                           const float* mu, const float* logvar, float max_len, const float* grad_out, void* dl, int64_t ldd, void* dlT,
                           int64_t ldT, float* dmu, float* dlogvar, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Device-side input pipeline: the encoded data set lives in HBM as uint8 indices [N, L]; a batch is the
 * rows `rows[0..B)` expanded to what MoleLoader.__getitem__ + default collate produce (data_loader.py:26-31): int64 indices
 * [B, L] and, when ohe != NULL, the float one-hot [B, L, C].
 */
int mvae_expand_indices(const uint8_t* store, const int64_t* rows, int B, int L, int C, int64_t* idx, float* ohe, void* stream);

/* The MOSES counterpart: the tokenised corpus lives in HBM in CSR form -- tokens uint8 [total] (ids without specials) and offsets int64
 * [N + 1] -- and ONE launch is the reference's collate (moses_train_distrib.py:127-135: sorted(data, key=len, reverse=True), which is
 * stable, then <bos> + ids + <eos>) followed by pad_sequence: batch member i is corpus row rows[i] (int64 [B], any order, repeats allowed),
 * its output row is rank_i = #{j : len_j > len_i} + #{j < i : len_j == len_i}, and
 *   x_pad [B, x_ld] int64: row rank_i = bos, the row's tokens, eos, then pad up to column T - 1 (columns T .. x_ld - 1 are not touched);
 *   lengths [B] int32: lengths[rank_i] = len_i + 2 -- descending, the precondition of every recurrent kernel here (mvae_rnn_*_desc.lengths);
 *   rows_sorted [B] int64 (optional): rows_sorted[rank_i] = rows[i], the corpus row behind each batch row;
 *   err [1] int32 (optional, the caller zeroes it): raised with atomicMax to 1 by a row with len + 2 > T -- only its first T columns are
 *     written and its length is reported as T -- and to 2 by a row id outside [0, N), which is collated as an empty row (bos, eos).
 * Nothing is ever written outside x_pad[:, :T], lengths[0..B) and rows_sorted[0..B); offsets must be a non-decreasing CSR index into tokens.
 * Any B >= 1 in one launch with no dependency between blocks.  Refused before anything is enqueued (MVAE_ERR_INVALID): a null tokens /
 * offsets / rows / x_pad / lengths, B < 1, T < 2, N < 1, x_ld < T, or bos / eos / pad outside [0, 65535].
 */
int mvae_moses_collate(const uint8_t* tokens, const int64_t* offsets, const int64_t* rows, int B, int T, int64_t N, int bos, int eos, int pad,
                       int64_t* x_pad, int64_t x_ld, int32_t* lengths, int64_t* rows_sorted, int32_t* err, void* stream);

/* An exact index of that corpus: which corpus row, if any, has exactly the tokens of a sampled row (the "novel" of valid / unique / novel).
 * Corpus row r is the byte string tokens[offsets[r] : offsets[r + 1]] of the CSR above; empty rows are legal.  The index is an
 * open-addressing hash table with linear probing: slots int64 [n_slots], allocated by the caller, n_slots a power of two greater than N,
 * so at least one slot is always empty and every probe sequence ends.  What the slots hold is opaque: only these two entries read them.
 * mvae_corpus_index_build: fills the table in one launch.  It sets every slot to empty itself (the caller need not clear anything) and
 *   zeroes n_distinct.  Every row is hashed over its token values and walks forward from its home slot: an empty slot is claimed by a
 *   compare-and-swap; at an occupied one the row is compared, byte for byte, with the occupant's, equal content leaves the lower row id
 *   in the slot (an atomic min), anything else moves on.  No thread waits for another and a walk takes at most n_slots steps.  Afterwards
 *   every distinct content owns exactly one slot, which names the LOWEST corpus row with that content, and n_distinct[0] (optional) is the
 *   number of distinct rows.  Which slot a content owns may depend on the order of execution; what mvae_corpus_index_probe and n_distinct
 *   return does not.  Building again into the same slots gives an equivalent table.
 * mvae_corpus_index_probe: one launch for a batch x [B, x_ld] int64 of token rows with <bos> in column 0 (x_ld >= T).  The content of row
 *   b is x[b, 1:] up to, and not including, the first column that holds `eos`; without one it runs to column T - 1 (a sample cut at
 *   max_len is compared by the tokens it has).  Nothing at or behind the <eos> takes part: whatever stands there -- ids outside the
 *   vocabulary, another row's tokens -- the answer is the same, and no column >= T is ever loaded.  match[b] = the lowest corpus row whose
 *   tokens equal that content, or -1.  A hash decides where to look and a 24-bit tag lets most foreign slots be passed unread, but a hit
 *   is always confirmed on the bytes: there are no false matches.  An id outside [0, 255] inside the content can equal no corpus token:
 *   the row gets -1 and the id is never used as an index.  T = 1, or `eos` in column 1, is the empty content and matches the lowest
 *   empty corpus row if there is one.  The walk is bounded by n_slots steps and checks every row id it finds against N, so a launch on
 *   slots that no build filled ends too, with meaningless answers.
 * Both refuse, before anything is enqueued (MVAE_ERR_INVALID): a null tokens / offsets / slots (/ x / match), N < 1 or N >= 2^40, n_slots
 * not a power of two or not greater than N; the probe also B < 1, T < 1, x_ld < T, eos outside [0, 65535].
 */
int mvae_corpus_index_build(const uint8_t* tokens, const int64_t* offsets, int64_t N, int64_t* slots, int64_t n_slots,
                            int64_t* n_distinct /* [1] or NULL */, void* stream);
int mvae_corpus_index_probe(const uint8_t* tokens, const int64_t* offsets, int64_t N, const int64_t* slots, int64_t n_slots, int B, int T,
                            const int64_t* x, int64_t x_ld, int eos, int64_t* match /* [B] */, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * MOSES GRU path (mosesvae.py:126-199).
 *   mvae_moses_latent_*: z = mu + exp(logvar/2)*eps and kl = 0.5*mean_b sum_j(exp(logvar) + mu^2 - 1 - logvar)  (mosesvae.py:158-162);
 *     backward adds dkl * d(kl) and an optional external dlogvar (logvar is a return value of VAE.forward).
 *   mvae_ce_loss_*: F.cross_entropy(y[:, :-1], x[:, 1:], ignore_index=pad) (mosesvae.py:193-197) on TIME-MAJOR logits
 *     (row t*B+b, leading dimension ldl); loss2[0] = loss, loss2[1] = number of counted tokens.  Backward writes dlogits in
 *     `dtype` with zero-padded columns V..ldd-1 (the next GEMM's K), adding an optional external dy given in [B,T,V] layout.
 *     A target outside [0, V) that is not pad is never read through: it makes loss2[0] NaN and is not counted in loss2[1], and its
 *     row's cross-entropy gradient is zero (the external dy is still added), so dlogits stays finite.
 *   mvae_permute102: [T,B,V] -> [B,T,V] (the `y` return value); mvae_relu_bwd: dy *= (y > 0) in place.
 *   mvae_mask_rows_tb: rows (t*B + b) with t >= lengths[b] of a time-major [T*B, ld] buffer := 0 (ld * sizeof(dtype) a multiple of 16).
 *     pad_packed_sequence (mosesvae.py:189) emits zeros at finished positions, so no gradient reaches h there: when an external gradient
 *     w.r.t. the returned logits was added to dl, those rows are cleared before mvae_rnn_bwd contracts dl as dy_a (the decoder_fc weight /
 *     bias gradients are taken from the unmasked dl first).
 */
size_t mvae_moses_latent_workspace(int B);     /* one float per sequence: per-row KL sums, added up in a fixed order */
/* eps == NULL: eps[i] = n(seed, offset + i) is drawn in the launch and written to eps_out (see mvae_lambda_fwd). */
int mvae_moses_latent_fwd(int B, int dz, const float* mu, const float* logvar, const float* eps, uint32_t seed, uint64_t offset, float* eps_out,
                          float* z, float* kl_out, void* ws, size_t ws_bytes, void* stream);
int mvae_moses_latent_bwd(int B, int dz, const float* mu, const float* logvar, const float* eps, const float* dz_in, const float* dkl,
                          const float* dlogvar_ext, float* dmu, float* dlogvar, void* stream);
/* Free-bits form of the latent pass (an addition: Kingma et al. 2016 in the per-dimension batch-mean form, against posterior collapse).
 * With k_bj = 0.5 (exp(logvar_bj) + mu_bj^2 - 1 - logvar_bj) and m_j = (1 / B) sum_b k_bj:
 *   kl_dim[j] = m_j  (fp32 [dz]),  kl2[0] = sum_j max(m_j, free_bits)  (the objective),  kl2[1] = sum_j m_j  (the KL itself, what
 *   mvae_moses_latent_fwd reports).  z and eps_out are written exactly as mvae_moses_latent_fwd writes them: the same draw for the same
 *   (seed, offset), z bitwise the same.  free_bits is in nats per latent dimension; a dimension costs nothing until it carries that much.
 * The column sums over the batch are two-stage and fixed-order (per-block partial sums in ws, one block finishes; no float atomics):
 * two calls give the same bits.  k_bj is evaluated as 0.5 ((exp(lv) - 1 - lv) + mu^2) with the bracket free of cancellation.
 * mvae_moses_latent_fb_bwd is mvae_moses_latent_bwd with the KL term of dimension j multiplied by [kl_dim[j] >= free_bits] -- `>=`, as
 * torch.clamp(min = free_bits) differentiates, so free_bits = 0 switches nothing off; kl_dim is what the forward wrote.
 * Any B >= 1, dz >= 1.  Refused before anything is enqueued: free_bits < 0 or NaN, a null operand, B < 1, dz < 1 (MVAE_ERR_INVALID);
 * ws_bytes < mvae_moses_latent_fb_workspace(B, dz) (MVAE_ERR_WORKSPACE). */
size_t mvae_moses_latent_fb_workspace(int B, int dz);
int mvae_moses_latent_fb_fwd(int B, int dz, const float* mu, const float* logvar, const float* eps, uint32_t seed, uint64_t offset, float* eps_out,
                             float free_bits, float* z, float* kl2, float* kl_dim, void* ws, size_t ws_bytes, void* stream);
int mvae_moses_latent_fb_bwd(int B, int dz, const float* mu, const float* logvar, const float* eps, const float* dz_in, const float* dkl,
                             const float* dlogvar_ext, const float* kl_dim, float free_bits, float* dmu, float* dlogvar, void* stream);
/* Word dropout on the decoder's input tokens (an addition: Bowman et al. 2016): x_out[b, t] = unk_id where position (b, t) is eligible and
 * not kept, x[b, t] otherwise (x, x_out int64 [B, T]; x_out may not alias x).  Eligible: 1 <= t <= lengths[b] - 2, i.e. never <bos>
 * (t = 0), the last input token (t = lengths[b] - 1: <eos>, which the decoder reads but predicts nothing from) or padding.  Kept:
 * keep_mask[b * T + t] != 0 when a mask is given (bytes [B, T]; parity tests), else mvae_dropout_keep(seed, b * T + t, p) -- the counter
 * is the flat position in the PADDED batch, so the draw of a sequence depends on the batch's width T.  No RNG state anywhere: the host
 * can restate the draw.  n_dropped (optional, device int32): the number of replaced positions, an integer sum (exact, order-free).
 * Refused before anything is enqueued (MVAE_ERR_INVALID): p outside [0, 1) or NaN, B < 1, T < 1, null x, lengths or x_out. */
int mvae_token_dropout(const int64_t* x, const int32_t* lengths, int B, int T, int unk_id, float p, uint32_t seed, const uint8_t* keep_mask,
                       int64_t* x_out, int32_t* n_dropped, void* stream);
size_t mvae_ce_loss_workspace(int B, int T);
int mvae_ce_loss_fwd(int B, int T, int V, const float* logits, int64_t ldl, const int64_t* x, int pad, float* loss2, void* ws, size_t ws_bytes,
                     void* stream);
int mvae_ce_loss_bwd(int dtype, int B, int T, int V, const float* logits, int64_t ldl, const int64_t* x, int pad, const float* loss2,
                     const float* grad_out, const float* dy_ext, void* dl, int64_t ldd, void* stream);
int mvae_permute102(int T, int B, int V, const float* in, float* out, void* stream);
/* One autoregressive sampling step behind the GRU step kernels (mosesvae.py:236-253): y = decoder_fc(h_top) (w_fc [V, ldw] dtype, V <= 64),
 * p = softmax(y / temp), w ~ multinomial(p, 1) with EXPLICIT randomness -- u(b) = hash(seed, step * B + b) / 2^32 with the counter hash of
 * mvae_dropout_keep; the sample is the first class k with cumsum_k(p) > u * sum(p) --, then the reference's bookkeeping
 * (x[b, step] = w unless the sequence has ended; a first <eos> sets end_pads[b] = step + 1 and eos_mask[b]) and the NEXT step's layer-0
 * addend row add_out[b] = table[w_b] + base[b] (fp32 [*, W], the embedding folded into the input projection).  w_out [B]: the sampled ids. */
int mvae_moses_sample_step(int dtype, int B, int V, int H, const void* h_top, int64_t ldh, const void* w_fc, int64_t ldw, const float* bias, float temp,
                           uint32_t seed, int step, int eos_id, const float* table, int W, const float* base, float* add_out, int64_t* x, int64_t x_ld,
                           int64_t* end_pads, uint8_t* eos_mask, int64_t* w_out, void* stream);
/* The filtered sibling of mvae_moses_sample_step (an addition: the reference samples from the full softmax only): top-k and nucleus (top-p)
 * truncation, the sample's log-probability under the distribution it was drawn from, and a running hash of the row's tokens.  Same shape
 * and constraints (V <= 64, the head must fit the LDS, bf16 and f32), one launch per generated token.  Per row b:
 *   1. p = softmax(decoder_fc(h_top[b]) / temp), with the fp32 arithmetic of mvae_moses_sample_step in the same order.
 *   2. The classes are ranked in the total order (p descending, class id ascending); before(v) = sum of p_u over the classes ranked before v.
 *   3. Keep set = {rank < top_k} (top_k == 0: off; valid 0 .. V) intersected with {before(v) < top_p * sum(p)}, i.e. the shortest rank
 *      prefix whose mass reaches top_p, the rank-0 class always kept (top_p >= 1: off; valid (0, 1], larger values mean off).  Both
 *      filters look at the unfiltered p: there is no renormalisation between them.
 *   4. q_v = keep_v ? p_v : 0; the sample w is the first kept class, in class-id order, with cumsum(q)_v > u * sum(q), u as in
 *      mvae_moses_sample_step.  With both filters off the tokens are bitwise those of mvae_moses_sample_step.
 *   5. Bookkeeping (x, end_pads, eos_mask), w_out and the next step's add_out row exactly as mvae_moses_sample_step.
 *   6. If the row had not ended before this step (the <eos> step itself counts): logq[b] += log(q_w / sum(q)) (fp32, exact logf) and
 *      hash[b] = (hash[b] ^ w) * 0x100000001b3 mod 2^64 -- 64-bit FNV-1a over the token ids x[b, 1 : end], one "byte" per id (<bos> is not
 *      hashed, <eos> is).  The caller initialises logq to 0 and hash to the FNV offset basis 0xcbf29ce484222325.  Either may be NULL.
 * Refused before anything is enqueued: what mvae_moses_sample_step refuses, with its codes, a dtype other than f32 / bf16, top_k outside
 * 0 .. V and top_p <= 0 or NaN (MVAE_ERR_INVALID). */
int mvae_moses_sample_filtered_step(int dtype, int B, int V, int H, const void* h_top, int64_t ldh, const void* w_fc, int64_t ldw, const float* bias,
                                    float temp, int top_k, float top_p, uint32_t seed, int step, int eos_id, const float* table, int W,
                                    const float* base, float* add_out, int64_t* x, int64_t x_ld, int64_t* end_pads, uint8_t* eos_mask,
                                    int64_t* w_out, float* logq /* [B] or NULL */, int64_t* hash /* [B] or NULL */, void* stream);
/* SMILES syntax (an addition): a small automaton over the tokens decides whether a character-level SMILES string is well-formed --
 * balanced branches, closed rings and brackets, no dangling bond, a bracket-atom grammar.  Syntax only: valence and aromaticity are not
 * checked.  It accepts a conservative subset of OpenSMILES: no %nn ring numbers, no '.', no isotopes, no "++" / "--", no ring digit
 * after a bond, at most 15 open branches; a ring may not close on the atom that opened it.  Accepted strings, with a = an organic-subset
 * atom (B C N O P S F I b c n o p s, Cl, Br), bond = one of = # : / \ -:
 *   chain   := atom ( ringdigit* ( bond? atom | '(' bond? chain ')' )* )*        every ring digit opened is closed on a later atom
 *   atom    := a | '[' ( a | 'H' ) '@'{0,2} ( 'H' digit? )? ( ('+'|'-') digit? )? ']'       ("[H" takes no chirality or H count)
 * Layouts (the tests build states with them):
 *   tok_info int32 [V], one word per token id: bits 0-7 the class -- 0 OTHER (never allowed: <bos>, <pad>, <unk>, unknown characters),
 *     1 ATOM, 2 TAIL ('l' / 'r'), 3 H, 4 BOND (= # : / \), 5 MINUS, 6 PLUS, 7 AT, 8 DIGIT, 9 LPAR, 10 RPAR, 11 LBRK, 12 RBRK, 13 EOS --,
 *     bits 8-15 for a TAIL the id of the token it must follow ('C' / 'B') plus 1, bits 16-19 for a DIGIT its value.
 *   state int32 [B, 2]: word 0 = mode | depth << 8 | prev_id << 16 (prev_id 0xFF: none), word 1 = open | cur << 16; depth = open
 *     branches, open = 10-bit mask of open ring digits, cur = mask of the ring digits already used on the current atom.  Modes: 0 START,
 *     1 ATOM, 2 ATOMX (after Cl / Br / ']'), 3 RING, 4 BOND, 5 OPEN, 6 CLOSE, 7 KOPEN ('['), 8 KSYM, 9 KSYMX, 10 KCHI1, 11 KCHI2, 12 KH,
 *     13 KHN, 14 KCHG, 15 KCHGN, 16 END, 17 ERROR.  The initial state is {0 | 0xFF << 16, 0}.
 * mvae_moses_sample_syntax_step: mvae_moses_sample_filtered_step constrained by the automaton.  For a row that had not ended, class v
 *   is allowed iff the automaton takes it from gstate[b] AND the tokens still needed to finish the string after it (<eos> included) fit
 *   the max_len - 1 - step that remain.  The stabilising max of the softmax runs over the allowed classes only, the others get
 *   probability 0; top-k / top-p rank the allowed classes among themselves (top_p of the legal mass); the draw, its "u rounded up"
 *   fallback (the last class kept AND allowed), logq (of the constrained distribution), hash and the bookkeeping are those of the
 *   filtered step; gstate[b] advances by the drawn token.  Some allowed token always lowers the need by one, so with max_len >= 3 the
 *   allowed set is never empty and every row draws <eos> by step max_len - 1; were it empty, the row emits <eos> and its mode becomes
 *   ERROR.  Rows that had ended are neither masked nor advanced.  Refused (MVAE_ERR_INVALID) before anything is enqueued: what the
 *   filtered entry refuses, a null tok_info or gstate, max_len < 3, step < 1, step >= max_len, eos_id outside [0, V).
 * mvae_smiles_syntax_check: one thread per row of x [B, T] int64 (bos first; x_ld >= T) runs the automaton over x[b, 1:] until <eos> is
 *   taken.  valid[b] = 1 iff it is; bad_pos[b] (optional) = the index of the first refused token (an id outside [0, V) is refused), T when
 *   the row ran out without <eos>, -1 when the row is valid.  eos_id is the only token that ends a row: it counts as EOS whatever
 *   tok_info says of it, and another id that tok_info calls EOS is refused.  V <= 64. */
int mvae_moses_sample_syntax_step(int dtype, int B, int V, int H, const void* h_top, int64_t ldh, const void* w_fc, int64_t ldw, const float* bias,
                                  float temp, int top_k, float top_p, uint32_t seed, int step, int eos_id, const float* table, int W,
                                  const float* base, float* add_out, int64_t* x, int64_t x_ld, int64_t* end_pads, uint8_t* eos_mask,
                                  int64_t* w_out, float* logq /* [B] or NULL */, int64_t* hash /* [B] or NULL */, const int32_t* tok_info /* [V] */,
                                  int32_t* gstate /* [B, 2] */, int max_len, void* stream);
/* Forced tokens in the sampling launch (prefix-constrained sampling, an addition): mvae_moses_sample_filtered_step (tok_info and gstate
 * NULL: the automaton is off) or mvae_moses_sample_syntax_step (both given) with a table forced int32 [B, forced_ld], forced_ld > step.
 * forced[b, step] in [0, V) is the token row b writes at this step instead of drawing one: no temperature, filter or mask is applied and
 * no random draw is consumed (the draw of a free step stays u(b) = hash(seed, step * B + b)).  The token goes through the bookkeeping of a
 * drawn one -- x[b, step] and end_pads / eos_mask unless the row had ended, hash[b] folded, gstate[b] advanced (mode ERROR if the automaton
 * refuses the token), w_out[b], add_out[b] = table[token] + base[b] -- and adds NOTHING to logq[b].  Any other value (-1 by convention)
 * leaves the row free: it gets, bit for bit, what the sibling launch writes.  Refused: what the sibling refuses (the syntax conditions only
 * when tok_info is given), a NULL forced, forced_ld <= step, exactly one of tok_info / gstate NULL (MVAE_ERR_INVALID). */
int mvae_moses_sample_forced_step(int dtype, int B, int V, int H, const void* h_top, int64_t ldh, const void* w_fc, int64_t ldw, const float* bias,
                                  float temp, int top_k, float top_p, uint32_t seed, int step, int eos_id, const float* table, int W,
                                  const float* base, float* add_out, int64_t* x, int64_t x_ld, int64_t* end_pads, uint8_t* eos_mask,
                                  int64_t* w_out, float* logq /* [B] or NULL */, int64_t* hash /* [B] or NULL */,
                                  const int32_t* tok_info /* [V] or NULL */, int32_t* gstate /* [B, 2] or NULL */, int max_len,
                                  const int32_t* forced /* [B, forced_ld], -1 = free */, int64_t forced_ld, void* stream);
/* mvae_smiles_prefix_state: one thread per row walks the automaton from its initial state over ids[b, 0 : lens[b]] (int32 [B, P], row
 * stride ids_ld >= P; lens clamped to 0 .. P).  state [B, 2] = the packed state reached, need [B] = the tokens still required to finish
 * the string from it (<eos> included), bad_pos [B] = the index of the first refused token (an id outside [0, V) is one), -1 if none; after
 * a refusal the state is the one in front of the refused token with mode ERROR, and need is 0.  V <= 64. */
int mvae_smiles_prefix_state(int B, int P, int V, const int32_t* ids, int64_t ids_ld, const int32_t* lens /* [B] */,
                             const int32_t* tok_info /* [V] */, int32_t* state /* [B, 2] */, int32_t* need /* [B] */, int32_t* bad_pos /* [B] */,
                             void* stream);
int mvae_smiles_syntax_check(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info /* [V] */, int eos_id,
                             uint8_t* valid /* [B] */, int32_t* bad_pos /* [B] or NULL */, void* stream);
/* Beam-search decoding (an addition beyond the reference, which only samples): R = B * K rows, molecule m owning rows m*K .. m*K + K-1.
 * mvae_moses_beam_step: one launch per generated token behind the GRU step.  logp = log_softmax(decoder_fc(h_top)) (w_fc [V, ldw] dtype,
 *   V <= 64 else MVAE_ERR_UNSUPPORTED; 1 <= K <= min(16, V) else MVAE_ERR_INVALID).  An active beam proposes its top-K tokens at
 *   score + logp, a finished beam (fin != 0) proposes itself once (token pad_id, score unchanged); per molecule the best K candidates
 *   survive in the order (score desc, parent beam asc, token asc), a NaN counting as -inf.  Per new beam r it writes score[r], fin[r],
 *   ends[r] (step + 1 at the first <eos>, unchanged otherwise: initialise ends to max_len), the backpointer record hist_tok / hist_par
 *   [max_len, R] int32 at row `step` (token; parent beam 0..K-1 of the same molecule), the next step's layer-0 addend row
 *   add_out[r] = table[token] + base[r] (fp32 [*, W], 16-byte aligned), and reorders the recurrent state: state (dtype) holds, per layer l
 *   (offset l * layer_stride elements), half 0 = the state the GRU step read as h0 and half 1 (offset half_stride) = the state it wrote,
 *   rows of ldh elements; the parent's half-1 row is copied into row r of half 0 for every layer.  h_top is half 1 of the last layer.
 *   Initial state: score 0 for beam 0 and -inf for beams 1..K-1 of every molecule, fin 0, ends max_len.
 * mvae_moses_beam_syntax_step: mvae_moses_beam_step over well-formed strings only (the automaton of "SMILES syntax" above).  gstate
 *   int32 [B*K, 2] holds the packed automaton state of every beam row, initially {0 | 0xFF << 16, 0}.  An active row may propose class v
 *   iff the automaton takes it from gstate[r] AND the tokens still needed to finish the string after it (<eos> included) fit the
 *   max_len - 1 - step that remain -- the rule of mvae_moses_sample_syntax_step; it proposes its best min(K, allowed) classes in the order
 *   (score desc, token asc).  The score is NOT renormalised: logp stays the log-softmax over all V classes and the mask only removes
 *   candidates, so a hypothesis' score is still log p(tokens | z) and the search returns the most probable well-formed strings the beam
 *   finds (sampling renormalises because it defines a distribution; decoding does not).  Finished rows (fin != 0) are neither masked
 *   nor advanced and propose themselves once.  gstate is reordered with the recurrent state: new row r with parent p gets p's old
 *   state if p was finished, else step(p's old state, token), mode ERROR if the step is refused (in place: a workgroup owns whole
 *   molecules).  A molecule can have fewer than K candidates (K = 16 at max_len = 3: one per atom token): a slot without one is dead --
 *   score -inf, parent 0, token pad_id, which puts its automaton in ERROR, so it proposes nothing again, stays at -inf and never
 *   outranks a finite hypothesis; its ids and ends are unspecified but deterministic.  Some allowed token always lowers the need by one,
 *   so an active state is never left without an allowed token: beam 0 of every molecule is finite and every finite hypothesis takes
 *   <eos> by step max_len - 1.  Refused (MVAE_ERR_INVALID) before anything is enqueued: what mvae_moses_beam_step refuses, a null
 *   tok_info or gstate, max_len < 3, step < 1, step >= max_len, eos_id outside [0, V); V > 64 stays MVAE_ERR_UNSUPPORTED.
 * mvae_moses_beam_finalize: ids [B, K, max_len] int64 from the backpointers (bos_id first, pad after each end), in score order (the beams
 *   are kept sorted by mvae_moses_beam_step); ends_out [B*K] / score_out [B*K] (optional) copy ends / score.
 * mvae_ce_rows_fwd: out[b] = log p(x[b] | z) = sum over t of log_softmax(logits row t*B+b)[x[b, t+1]] for x[b, t+1] != pad -- the targets of
 *   mvae_ce_loss_fwd, one float per sequence, summed in t order (bitwise deterministic); an id outside [0, V) gives NaN. */
int mvae_moses_beam_step(int dtype, int B, int K, int V, int H, int layers, void* state, int64_t layer_stride, int64_t half_stride, int64_t ldh,
                         const void* w_fc, int64_t ldw, const float* bias, int step, int eos_id, int pad_id, const float* table, int W,
                         const float* base, float* add_out, float* score, uint8_t* fin, int64_t* ends, int32_t* hist_tok, int32_t* hist_par,
                         void* stream);
int mvae_moses_beam_syntax_step(int dtype, int B, int K, int V, int H, int layers, void* state, int64_t layer_stride, int64_t half_stride,
                                int64_t ldh, const void* w_fc, int64_t ldw, const float* bias, int step, int eos_id, int pad_id, const float* table,
                                int W, const float* base, float* add_out, float* score, uint8_t* fin, int64_t* ends, int32_t* hist_tok,
                                int32_t* hist_par, const int32_t* tok_info /* [V] */, int32_t* gstate /* [B*K, 2] */, int max_len, void* stream);
/* Forced tokens in the beam launch (prefix-constrained decoding): mvae_moses_beam_step (tok_info and gstate NULL) or
 * mvae_moses_beam_syntax_step (both given) with a table forced int32 [B, forced_ld], one row per MOLECULE, forced_ld > step.  With
 * forced[m, step] in [0, V) every active beam of molecule m proposes exactly one candidate, that token at score + logp[token] (logp the
 * log-softmax over all V classes: the score stays log p(tokens | z), prefix included); under the automaton the token is not masked, the
 * state advances with it and a refused token puts it in ERROR.  The beams that were dead (-inf) stay dead through the forced steps and
 * come alive at the first free one, as they do at step 1.  Any other value (-1) leaves the molecule free: bit for bit the sibling launch.
 * Refused: what the sibling refuses, a NULL forced, forced_ld <= step, exactly one of tok_info / gstate NULL (MVAE_ERR_INVALID). */
int mvae_moses_beam_forced_step(int dtype, int B, int K, int V, int H, int layers, void* state, int64_t layer_stride, int64_t half_stride,
                                int64_t ldh, const void* w_fc, int64_t ldw, const float* bias, int step, int eos_id, int pad_id, const float* table,
                                int W, const float* base, float* add_out, float* score, uint8_t* fin, int64_t* ends, int32_t* hist_tok,
                                int32_t* hist_par, const int32_t* tok_info /* [V] or NULL */, int32_t* gstate /* [B*K, 2] or NULL */, int max_len,
                                const int32_t* forced /* [B, forced_ld], -1 = free */, int64_t forced_ld, void* stream);
int mvae_moses_beam_finalize(int B, int K, int max_len, int bos_id, const int32_t* hist_tok, const int32_t* hist_par, const int64_t* ends,
                             const float* score, int64_t* ids, int64_t* ends_out, float* score_out, void* stream);
int mvae_ce_rows_fwd(int B, int T, int V, const float* logits, int64_t ldl, const int64_t* x, int pad, float* out, void* stream);
int mvae_relu_bwd(int64_t n, float* dy, const float* y, void* stream);
int mvae_mask_rows_tb(int dtype, int T, int B, int64_t ld, const int32_t* lengths, void* buf, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Latent diagnostics of mosesvae.VAE (an addition: the reference's trainer has no evaluation of its latent code): the importance-weighted
 * log-likelihood, the mutual information I(x; z) under the encoder (He et al. 2019, calc_mi, over the whole evaluated set) and, on the host,
 * the active units.  fp32 throughout; every reduction runs in a fixed order without atomics (two runs are bitwise equal).  Sizes < 1,
 * a leading dimension < dz or a NULL pointer an argument needs give MVAE_ERR_INVALID before anything is enqueued.
 * mvae_gauss_iw_draw: K draws per molecule from q(z | x) = N(mu_b, exp(logvar_b)) (mu, logvar [B, ld]): row r = b*K + k of z_out [B*K, dz]
 *   is z = mu_b + exp(logvar_b / 2) * eps_r and logw_out[r] = 0.5 * sum_d (eps^2 + logvar - z^2) = log N(z; 0, I) - log N(z; mu, sigma^2).
 *   eps == NULL: eps_rd = n(seed, offset + r*dz + d), the counter normal of mvae_lambda_fwd; else eps is read from [B*K, dz].
 * mvae_group_logmeanexp: per group g of K values v_k = a[gK + k] + b[gK + k] (b may be NULL): lme_out[g] = m + log sum_k exp(v_k - m) - log K
 *   with m = max_k v_k, and mean_out[g] = sum_k v_k / K.  A NaN makes its own group's lme NaN; an all -inf group gives -inf.
 * mvae_gauss_pairwise_lse: out[i] = logsumexp_j log N(z_i; mu_j, exp(logvar_j)) over Nx diagonal Gaussians (mu, logvar [Nx, ldp]) for Nz
 *   points (z [Nz, ldz]) -- a direct difference per (pair, dimension), not an expanded square.  dz <= 192 (else MVAE_ERR_UNSUPPORTED).
 *   Workspace: mvae_gauss_pairwise_lse_workspace(Nz, Nx, dz) bytes (8-byte aligned; 0: none needed), else MVAE_ERR_WORKSPACE.
 */
int mvae_gauss_iw_draw(int B, int K, int dz, const float* mu, const float* logvar, int64_t ld, const float* eps, uint32_t seed, uint64_t offset,
                       float* z_out, float* logw_out, void* stream);
int mvae_group_logmeanexp(int G, int K, const float* a, const float* b, float* lme_out, float* mean_out, void* stream);
size_t mvae_gauss_pairwise_lse_workspace(int Nz, int Nx, int dz);
int mvae_gauss_pairwise_lse(int Nz, int Nx, int dz, const float* z, int64_t ldz, const float* mu, const float* logvar, int64_t ldp, float* out,
                            void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Exact k nearest neighbours in latent space (an addition: the table is the encoder mean of every corpus row, data.MosesLatentIndex).
 * mvae_latent_knn: for each of Q queries (q [Q, ldq]) the k rows of table [N, ldt] at the smallest squared Euclidean distance
 *   d2(i, j) = sum_d (q[i,d] - table[j,d])^2, computed in fp32 as a sum of squares of fp32 differences -- no norm expansion, so a row's
 *   distance to itself is exactly 0 and close neighbours keep their order.  The order of the sum is fixed (it does not depend on Q, N, k
 *   or on how the launch is laid out).
 *   Row i of dist / idx ([Q, k], dense) holds the k eligible rows with the smallest (d2, j), ascending in that pair: equal distances rank
 *   by the lower row index.  A row is eligible unless it is exclude[i] (exclude [Q] int64 or NULL; -1 = none) or its distance is NaN; a
 *   distance that overflowed to +inf is eligible.  With fewer than k eligible rows the tail of the output row is (+inf, -1).  Every element
 *   of dist and idx is written, nothing else is; two runs are bitwise equal.
 *   Nothing of size Q x N exists: one scan launch keeps a k-entry list per (query, wave) in LDS, and, when the table rows are split over
 *   `slots` partial lists per query to fill the chip (slots depends on Q and N alone, <= 256), one merge launch combines them by (d2, j).
 *   Workspace: mvae_latent_knn_workspace(Q, N, dz, k) = slots * Q * k * 12 bytes (8-byte aligned; 0: one slot, none needed).
 *   Limits: dz <= 192 and k <= 32, else MVAE_ERR_UNSUPPORTED (the workspace function then returns 0).  Q, N, k or dz < 1, a leading
 *   dimension < dz or a NULL pointer other than exclude give MVAE_ERR_INVALID, a short or missing workspace MVAE_ERR_WORKSPACE; all of
 *   these before anything is enqueued.
 */
size_t mvae_latent_knn_workspace(int Q, int64_t N, int dz, int k);
int mvae_latent_knn(int Q, int64_t N, int dz, int k, const float* q, int64_t ldq, const float* table, int64_t ldt, const int64_t* exclude,
                    float* dist, int64_t* idx, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Token-level Levenshtein distance (an addition: how far two strings are apart, where mvae_corpus_index_probe only says equal or not, and
 * the model-free counterpart of mvae_latent_knn).
 * Content of a row, the convention of mvae_corpus_index_probe: for a row r of an int64 [*, T] tensor it is r[1:] up to, and not including,
 *   the first column equal to `eos`; without one it runs to column T - 1.  Column 0 (<bos>) is never part of it and its value does not
 *   matter; nothing at or behind the <eos> takes part -- whatever stands there, the answer is the same -- and no column >= T is ever
 *   loaded.  T = 1, or `eos` in column 1, is the empty content.  Corpus row j is the byte string tokens[offsets[j] : offsets[j + 1]] of the
 *   CSR above; empty rows are legal, and only bytes inside tokens[0 : offsets[N]) are ever loaded.
 * Distance: plain Levenshtein with unit costs for insert, delete and substitute, no transposition.  Token p of the pattern side and token
 *   t of the text side are equal iff p == t and 0 <= p < V: an id outside [0, V) on either side -- a corpus byte >= V, a negative id, an
 *   int64 far out of range -- equals nothing, not even itself, and is never used as an index.  The distance between contents of lengths
 *   m and n is exact (a bit-parallel dynamic program in 64-bit words, one word for m <= 64, two with a carry for m <= 128), lies between
 *   |m - n| and max(m, n) and is returned as int32.
 * mvae_edit_distance_rows: dist[i] = the distance between the content of a[i] ([B, a_ld] int64, Ta columns) and the content of b[i]
 *   ([B, b_ld], Tb columns), one launch.  a is the pattern side: Ta - 1 <= MVAE_EDIT_PATTERN_MAX, else MVAE_ERR_UNSUPPORTED; Tb is
 *   unlimited.  Exactly dist[0..B) is written.
 * mvae_edit_knn: for each of Q queries (x [Q, x_ld] int64, T columns; the pattern side, T - 1 <= MVAE_EDIT_PATTERN_MAX) row i of dist /
 *   idx ([Q, k], dense) holds the k eligible corpus rows with the smallest (distance, row), ascending in that pair: equal distances rank
 *   by the lower row, so a query whose content equals a corpus row gets (0, lowest such row) first -- mvae_corpus_index_probe's answer.
 *   Every corpus row is eligible except exclude[i] (exclude [Q] int64 or NULL; -1 = none).  With fewer than k eligible rows the tail of
 *   the output row is (MVAE_EDIT_NONE, -1).  Every element of dist and idx is written, nothing else is.  A query's answer does not depend
 *   on Q, on the other queries or on how the launch is laid out; two runs are equal.
 *   Nothing of size Q x N exists: one scan launch keeps a k-entry list per (query, wave) in LDS, and, when the corpus rows are split
 *   over `slots` partial lists per query to fill the chip (slots depends on Q and N alone, <= 256), one merge launch combines them by
 *   (distance, row).  Workspace: mvae_edit_knn_workspace(Q, N, k) = slots * Q * k * 12 bytes (8-byte aligned; 0: one slot, none needed);
 *   it depends on (Q, N, k) alone.
 * Refused before anything is enqueued.  MVAE_ERR_INVALID: a NULL pointer other than exclude; B, Q, N, k, T, Ta or Tb < 1; a leading
 *   dimension below its T; eos outside [0, 65535]; V outside [1, 64].  MVAE_ERR_UNSUPPORTED: k > 32, or a pattern side wider than 129
 *   columns (the workspace function then returns 0).  MVAE_ERR_WORKSPACE: a missing or short workspace.
 */
#define MVAE_EDIT_NONE 2147483647      /* distance of an empty k-NN entry */
#define MVAE_EDIT_PATTERN_MAX 128      /* longest content on the pattern side */
int mvae_edit_distance_rows(int B, int V, int eos, const int64_t* a, int64_t a_ld, int Ta, const int64_t* b, int64_t b_ld, int Tb,
                            int32_t* dist /* [B] */, void* stream);
size_t mvae_edit_knn_workspace(int Q, int64_t N, int k);
int mvae_edit_knn(int Q, int T, int V, int eos, const int64_t* x, int64_t x_ld, const uint8_t* tokens, const int64_t* offsets, int64_t N, int k,
                  const int64_t* exclude /* [Q] or NULL, -1 = none */, int32_t* dist /* [Q, k] */, int64_t* idx /* [Q, k] */, void* ws,
                  size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * SMILES graph (an addition: "SMILES syntax" above decides whether a row is well-formed and says that valence is not its business; this is
 * the second automaton on top of it).  The token row is parsed into its molecular graph, the valence rules and the graph rules that need
 * no kekulisation are enforced, and per-row integers come out: a status, the heavy-atom / bond / ring / hydrogen counts, the molecular
 * formula.  Status 0 is a NECESSARY condition for chemical validity, not a sufficient one: it means correct valences, sane ring bonds and
 * aromatic atoms in rings.  It does not test whether an aromatic system kekulises and it does not reject c1(C)(C)cccc1; a row with
 * status 0 is "valence-consistent", which is less than what a cheminformatics toolkit calls valid.
 * Input language: exactly what the syntax automaton accepts.  Under that grammar a ring digit never follows a bond, there is no '.', and
 *   no isotopes: ring-closure bonds are always implicit and the graph is connected.
 * Elements, in this order (MVAE_SMILES_ELEMENTS = 11): H B C N O F P S Cl Br I; a lower-case atom is the aromatic form of its element.
 * Bond contribution: '=' counts 2, '#' counts 3, every other bond counts 1 -- implicit, - : / \ and ring closures.  Aromatic bonds count 1
 *   on purpose (the hydrogen rule of OpenSMILES); nothing kekulises.  '@' is ignored.
 * chem_info int32 [V], one word per token id beside tok_info: bits 0-3 the element (ATOM and H tokens: the token's element; a TAIL: the
 *   element the pair spells, Cl or Br), bit 4 the aromatic flag, bits 8-9 the bond order of a BOND or MINUS token.
 * The walk: the row goes through smi::step.  A row the automaton refuses, or one without <eos>, gets status SYNTAX and the bad_pos of
 *   mvae_smiles_syntax_check, whatever else the row holds.  Alongside, the graph:
 *   - an organic-subset atom comes into being at its ATOM token; a TAIL token (l, r) changes the element of the current atom (C -> Cl,
 *     B -> Br) and re-checks it; a bracket atom comes into being at its ']', with H count 1 for 'H' and the digit for 'Hn', and charge
 *     sign * (digit if present, else 1).  [H] is a graph node of element H.
 *   - a new atom gets a bond of the pending order to the current atom, if there is one; the pending order is set by a bond token and
 *     defaults to 1.  '(' pushes the current atom, ')' pops it back to current.
 *   - an opening ring digit records the current atom.  A closing digit on atom j with opener i first checks for a duplicate bond -- i is
 *     j's tree predecessor, or (i, j) were already joined by another digit: status RING_BOND --, otherwise adds a bond of 1 to both atoms
 *     and marks as ring members every atom on the tree path i .. j through their lowest common ancestor.
 *   - after every update of an atom (creation, new bond, tail) its used valence U = sum of bond contributions + bracket H count is
 *     checked against the largest allowed valence of (element, charge); exceeding it gives status VALENCE.  Unbracketed atoms have
 *     charge 0.  A bracket atom with |charge| >= 2, or with no table entry, gets status CHARGE at its ']' -- decided before the atom is
 *     bonded, so CHARGE wins over a VALENCE the same ']' would raise.  Allowed valences (charge -1 / 0 / +1; - = no entry):
 *       H {0} {1} {0}    B {4} {3} -     C {3} {4} {3}    N {2} {3} {4}        O {1} {2} {3}      F {0} {1} -
 *       P {2} {3,5} {4}  S {1} {2,4,6} {3,5}              Cl {0} {1} -         Br {0} {1} -       I {0} {1,3,5} -
 *   - at <eos>: a well-formed row with more than 127 content tokens gets status TOO_LONG (bad_pos the <eos> column) and nothing else is
 *     reported for it; else the first graph error in token order stands; else an aromatic atom that is no ring member gives status
 *     AROMATIC with bad_pos the <eos> column.
 *   bad_pos: for SYNTAX what mvae_smiles_syntax_check gives; for VALENCE / CHARGE / RING_BOND the column of the token being processed
 *     when the first error was found (both ends of a new bond are checked at that one token); -1 for status 0.
 *   Implicit hydrogens, unbracketed atoms only: with S the atom's bond sum and v0 the smallest allowed valence (charge 0) >= S, an
 *     aliphatic atom has v0 - S, an aromatic one max(0, v0 - S - 1).  Bracket atoms have none beyond their H count.
 * Status: 0 OK, 1 SYNTAX, 2 VALENCE, 3 CHARGE, 4 RING_BOND, 5 AROMATIC, 6 TOO_LONG.
 * Outputs, per row: status int32 [B]; bad_pos int32 [B] (optional); desc int32 [B, 8] (optional) = heavy atoms (nodes that are not H),
 *   bonds, rings (= bonds - nodes + 1), ring atoms, aromatic atoms, hydrogens (implicit + bracket counts + [H] nodes), net charge, hetero
 *   atoms (heavy, not C); formula int32 [B, 11] (optional) = atoms per element in the order above, slot 0 the hydrogens.  A row whose
 *   status is not 0 gets zeros in desc and formula.  Every element of the given outputs is written, nothing else is.
 * mvae_smiles_graph_rows: one thread per row of x [B, T] int64 (bos first; x_ld >= T); eos_id and ids outside [0, V) are treated exactly
 *   as mvae_smiles_syntax_check treats them.
 * mvae_smiles_graph_corpus: the same over the CSR corpus (uint8 rows without specials, tokens[offsets[j] : offsets[j + 1]]): the end of the
 *   row acts as <eos>, bad_pos is 0-based in the row (the row's length for the <eos> column), an empty row gets SYNTAX at 0.
 * mvae_smiles_graph_host: mvae_smiles_graph_rows on HOST pointers, a plain loop over the rows through the same source compiled for the
 *   CPU (the precedent of mvae_dropout_keep and mvae_normal_words): the parse can be tested and sanitised without a device.
 * Refused before anything is enqueued: V > 64 (MVAE_ERR_UNSUPPORTED); a NULL x / tokens / offsets / tok_info / chem_info / status, B, N, T
 *   or V < 1, x_ld < T, eos_id outside [0, V) (MVAE_ERR_INVALID).
 */
#define MVAE_SMILES_ELEMENTS 11
#define MVAE_SMILES_DESC 8
#define MVAE_SMILES_CONTENT_MAX 127    /* content tokens of a row the graph is kept for */
int mvae_smiles_graph_rows(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info /* [V] */, const int32_t* chem_info /* [V] */,
                           int eos_id, int32_t* status /* [B] */, int32_t* bad_pos /* [B] or NULL */, int32_t* desc /* [B, 8] or NULL */,
                           int32_t* formula /* [B, 11] or NULL */, void* stream);
int mvae_smiles_graph_corpus(const uint8_t* tokens, const int64_t* offsets /* [N + 1] */, int64_t N, int V, const int32_t* tok_info /* [V] */,
                             const int32_t* chem_info /* [V] */, int32_t* status /* [N] */, int32_t* bad_pos /* [N] or NULL */,
                             int32_t* desc /* [N, 8] or NULL */, int32_t* formula /* [N, 11] or NULL */, void* stream);
int mvae_smiles_graph_host(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info /* [V] */, const int32_t* chem_info /* [V] */,
                           int eos_id, int32_t* status /* [B] */, int32_t* bad_pos /* [B] or NULL */, int32_t* desc /* [B, 8] or NULL */,
                           int32_t* formula /* [B, 11] or NULL */);

/* ---------------------------------------------------------------------------------------------------------
 * Circular fingerprint (an addition: a second consumer of the "SMILES graph" walk above).  A 1024-bit circular fingerprint of radius 2,
 * built like ECFP4 but NOT rdkit's Morgan fingerprint: the bits are this library's own, nothing is kekulised, and two toolkits' bit
 * vectors are not comparable -- "shares most substructures" within this library, in the same sense in which status 0 is
 * "valence-consistent" and not what a toolkit calls valid.  Not Morgan, not kekulised.
 * It is defined on the graph exactly as the walk builds it.  Ring-closure bonds are order 1, as they are there.  All arithmetic is
 *   mod 2^32.
 * mix.  mix(h) is: h ^= h >> 16; h *= 0x85ebca6b; h ^= h >> 13; h *= 0xc2b2ae35; h ^= h >> 16.
 * Atom invariant.  For atom a, w(a) = elem | arom << 4 | (charge + 1) << 5 | in_ring << 7 | degree << 8 | used << 12.
 *   - elem is the index into H B C N O F P S Cl Br I.
 *   - degree is the number of graph neighbours.  Explicit [H] atoms are atoms.
 *   - used is the final used valence: the sum of bond orders plus bracket hydrogens (what the atom word holds at <eos>).
 *   - in_ring is the bit of the walk's ring mask.
 *   - id_0(a) = mix(w(a)).
 * Bond type.  For a bond between a and b, bt is 4 if its order is 1 and both ends are aromatic atoms.  Otherwise bt is the order.
 * Rounds r = 1, 2.  id_r(a) = mix(id_{r-1}(a) * 0x9E3779B1 + r + SUM_{b in nbrs(a)} mix(id_{r-1}(b) ^ (bt(a,b) * 0x7FEB352D))).
 *   - The neighbour sum is commutative.  Nothing is sorted.
 *   - The result does not depend on how the atoms are numbered.
 * Bits.  For every atom and every r in {0, 1, 2}, set bit id_r(a) & 1023.
 *   - Bit b lives in word b >> 6, bit b & 63.
 *   - A fingerprint is MVAE_FP_WORDS = 16 int64 words, 128 B.
 *   - ECFP's duplicate-substructure removal is deliberately omitted.
 * Rows that are not OK.  A row whose status is not OK (syntax, valence, charge, ring bond, aromatic, too long) gets an all-zero
 *   fingerprint.  Status and fingerprint are written together: status int32 [B] as the graph entries give it, fp int64 [B, 16]; every
 *   element of both is written, nothing else is.
 * mvae_smiles_fp_rows / _corpus / _host: the inputs of mvae_smiles_graph_rows / _corpus / _host (padded int64 rows; the CSR corpus in one
 *   launch; the same source compiled for the CPU, on host pointers).  One thread per row; 112 KiB of LDS per 64-row block.
 * Refused before anything is enqueued: what the graph entries refuse (V > 64: MVAE_ERR_UNSUPPORTED; the rest MVAE_ERR_INVALID), and a
 *   NULL fp.
 */
#define MVAE_FP_WORDS 16
int mvae_smiles_fp_rows(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info /* [V] */, const int32_t* chem_info /* [V] */,
                        int eos_id, int32_t* status /* [B] */, int64_t* fp /* [B, 16] */, void* stream);
int mvae_smiles_fp_corpus(const uint8_t* tokens, const int64_t* offsets /* [N + 1] */, int64_t N, int V, const int32_t* tok_info /* [V] */,
                          const int32_t* chem_info /* [V] */, int32_t* status /* [N] */, int64_t* fp /* [N, 16] */, void* stream);
int mvae_smiles_fp_host(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info /* [V] */, const int32_t* chem_info /* [V] */,
                        int eos_id, int32_t* status /* [B] */, int64_t* fp /* [B, 16] */);

/* ---------------------------------------------------------------------------------------------------------
 * Murcko scaffold (an addition: a third consumer of the "SMILES graph" walk above).  The Bemis-Murcko framework of a row -- its rings,
 * the linkers between them, and the atoms double-bonded to either -- as a set of the row's atoms.  It is defined on the graph exactly as
 * the walk builds it: explicit [H] are atoms, ring-closure bonds are order 1, nothing is kekulised, '@' '/' '\' carry no information.  So
 * this is NOT rdkit's MurckoScaffold: the atom sets agree where the two graphs agree, but no scaffold SMILES is produced here
 * ("Scaffold SMILES" below writes one), nothing is sanitised, and the keys below are this library's own.  Not rdkit, not kekulised.
 * Atoms are numbered in string order (the order in which the walk creates them), from 0; a row has at most 127.
 * Core.  The ring atoms (the walk's ring mask: the atoms that lie on a cycle), plus every non-ring atom that lies on a path between two
 *   ring atoms.  Equivalently: what is left after repeatedly deleting atoms with at most one remaining neighbour.  Equivalently: a non-ring
 *   atom belongs to Core iff at least two of the components left when it is removed contain a ring atom.
 * Exo.  The atoms outside Core joined to a Core atom by a bond of order 2: the =O of a ring or linker carbonyl, both =O of a linker
 *   sulfonyl, an exocyclic =C.  (rdkit keeps these too.)
 * S = Core u Exo, with the bonds of the row that join two atoms of S.  A row with no ring has the empty scaffold.
 * Ring bond.  A bond is a ring bond iff it lies on a cycle: every closure bond, and every tree bond k - pred(k) that some closure's
 *   tree path (the path between its two ends through their lowest common ancestor) steps over.
 *
 * Graph key (an addition).  A 64-bit key of an atom subset U of a row with its induced bonds, equal for equal graphs however the string
 * spells them.  All arithmetic is mod 2^32; mix and the bond type bt are the "Circular fingerprint" section's.
 *   id_0(a) = mix(w_U(a)).
 *   For r = 1 .. MVAE_GRAPH_KEY_ROUNDS (= 8):
 *     id_r(a) = mix(id_{r-1}(a) * 0x9E3779B1 + r + SUM_{b in nbrs_U(a)} mix(id_{r-1}(b) ^ (bt'(a,b) * 0x7FEB352D))),
 *     bt'(a,b) = bt(a,b) + 8 * ring_bond(a,b).  The ring-bond bit is what tells decalin from bicyclopentyl, which neighbour refinement
 *     on atom invariants alone cannot separate.  nbrs_U(a): the neighbours of a that are in U.
 *   lo = mix(|U| * 0x9E3779B1 + SUM_{a in U} mix(id_8(a)));  hi = mix(bonds(U) * 0x85EBCA6B + SUM_{a in U} mix(id_8(a) ^ 0x5BD1E995)).
 *   key = lo | hi << 32 as int64; a result of 0 becomes 1.  0 means "none": U is empty, or the row is not OK.
 *   Molecule key: U = all atoms, w_U(a) = the fingerprint's w(a) (element, aromatic flag, charge, ring membership, degree, used valence).
 *   Scaffold key: U = S, w_S(a) = elem | arom << 4 | (charge + 1) << 5 | in_ring << 7 | deg_S(a) << 8, deg_S the number of neighbours in S.
 *     The used valence is left out, because removing substituents changes it: benzene, toluene and phenol have one scaffold key.
 *   Ring membership and ring bonds are those of the whole row in both keys.  Stereochemistry is ignored.
 *   What the keys promise.  Equal graphs always get equal keys.  Different graphs get different keys except for collisions of the 64-bit
 *     hash and for graphs that 8 rounds of neighbour refinement with these invariants cannot separate (regular graphs of equal degree
 *     and ring-bond pattern, for example).  tests/test_scaffold_host.py lists what is known to be separated.  This is not a canonical
 *     SMILES, and "distinct graphs" counted on these keys is a lower bound in that sense.
 * Outputs, per row: status int32 [B] as the graph entries give it; mask int64 [B, 2] (optional, may be NULL): bit a of word a >> 6 = atom
 *   a is in S; desc int32 [B, 4] = |S|, bonds of S, linker atoms (Core minus the ring atoms), |Exo|; key int64 [B, 2] = molecule key,
 *   scaffold key.  Every element of the given outputs is written, nothing else is.  A row whose status is not 0 gets zeros everywhere; a
 *   row with status 0 and no ring gets zeros except for its molecule key.
 * mvae_smiles_scaffold_rows / _corpus / _host: the inputs of mvae_smiles_fp_rows / _corpus / _host.  One thread per row;
 *   MVAE_SCAFFOLD_LDS_BYTES = 81920 B (80 KiB) of LDS per 64-row block, so that two blocks fit a CU: the atom words, whose storage
 *   becomes the neighbour sums once they are packed (32 KiB), the ids (32 KiB), and the packed atoms with the closure pairs (16 KiB).
 *   The two keys of a row run 16 refinement rounds in all.
 * Refused before anything is enqueued: what the fingerprint entries refuse (V > 64: MVAE_ERR_UNSUPPORTED; the rest MVAE_ERR_INVALID),
 *   and a NULL desc or key.
 */
#define MVAE_GRAPH_KEY_ROUNDS 8
#define MVAE_SCAFFOLD_DESC 4
#define MVAE_SCAFFOLD_LDS_BYTES 81920
int mvae_smiles_scaffold_rows(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info /* [V] */,
                              const int32_t* chem_info /* [V] */, int eos_id, int32_t* status /* [B] */, int64_t* mask /* [B, 2] or NULL */,
                              int32_t* desc /* [B, 4] */, int64_t* key /* [B, 2] */, void* stream);
int mvae_smiles_scaffold_corpus(const uint8_t* tokens, const int64_t* offsets /* [N + 1] */, int64_t N, int V, const int32_t* tok_info /* [V] */,
                                const int32_t* chem_info /* [V] */, int32_t* status /* [N] */, int64_t* mask /* [N, 2] or NULL */,
                                int32_t* desc /* [N, 4] */, int64_t* key /* [N, 2] */, void* stream);
int mvae_smiles_scaffold_host(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info /* [V] */,
                              const int32_t* chem_info /* [V] */, int eos_id, int32_t* status /* [B] */, int64_t* mask /* [B, 2] or NULL */,
                              int32_t* desc /* [B, 4] */, int64_t* key /* [B, 2] */);

/* ---------------------------------------------------------------------------------------------------------
 * Kekulisation (an addition: a fourth consumer of the "SMILES graph" walk above).  The graph, fingerprint and scaffold entries give status
 * 0 to a row whose aromatic system cannot be written with alternating single and double bonds -- c1cccn1 (pyrrole without its H),
 * c1cccc1, c1(C)(C)cccc1 --, and they keep doing so.  The entries below add that test: a row they give status 0 is "kekulisable", a
 * tighter necessary condition for chemical validity than "valence-consistent", and still no sufficient one.
 * What this is NOT: it is not rdkit's Kekulize or SanitizeMol, and agreement with either is neither tested nor claimed.  No aromaticity
 *   perception is done (no Hueckel count: c1ccc1 and c1ccccccc1 pass); radicals are not diagnosed (a bracket [c] with two ring bonds
 *   passes); no Kekule form is written and no other entry sees the bond orders found.  (The entries of "Aromatic normal form" below do
 *   perceive aromaticity, and refuse c1ccc1 and c1ccccccc1 with MVAE_SMILES_NOT_AROMATIC.)
 * It is defined on the graph exactly as the walk builds it, with the walk's own valence table ("SMILES graph").
 *   U(a): the atom's final used valence, as the atom word holds it at <eos>: the sum of bond contributions (aromatic bonds count 1) plus
 *     bracket hydrogens.
 *   v0(a): the smallest allowed valence of (element, charge) that is >= U(a).  Unbracketed atoms have charge 0.
 *   N: the aromatic atoms with v0(a) - U(a) >= 1 -- the atoms that take exactly one ring double bond.  This is the condition under which
 *     the implicit-hydrogen rule max(0, v0 - S - 1) already reserves one valence unit, so the double bond never exceeds v0 and the
 *     hydrogen counts of the graph entries stay right.  In N: c with two or three sigma bonds, pyridine n, [n+] with three neighbours,
 *     [nH+], [cH].  Not in N: [nH], n(C), o, s, c(=O), [n-], [cH-], c with four sigma bonds.
 *   E: the bonds of bond type 4 ("Circular fingerprint": order 1, both ends aromatic) that are ring bonds ("Murcko scaffold") and have
 *     both ends in N.  The bond between the rings of c1ccccc1c1ccccc1 is not in E.  A bond between two aromatic atoms that closes a
 *     NON-aromatic ring (the five-ring of fluorene written with lower-case atoms on both sides) IS in E, because the walk does not know
 *     which ring is aromatic; an extra edge can only help a matching, so this errs towards passing.
 *   A row whose walk status is 0 kekulises iff the graph (N, E) has a perfect matching; else it gets status MVAE_SMILES_KEKULE = 7.  A row
 *     whose walk status is not 0 keeps that status.  A row without aromatic atoms kekulises trivially.  (N, E) is a general graph --
 *     aromatic systems contain odd rings -- and the matching is a maximum matching, exact (Edmonds' blossom algorithm).
 * Outputs, per row: status int32 [B] (0 - 6 as the graph entries give it, or 7); desc int32 [B, 4] = |N|, |E|, pairs (the size of a
 *   maximum matching of (N, E)), deficiency (|N| - 2 * pairs), for status 0 AND status 7, zeros for any other status -- all four are
 *   determined by the row alone; mate uint8 [B, 128] (optional, may be NULL): mate[a] is the partner of atom a (string order) in the
 *   maximum matching found, 255 for an atom that is not matched or not in N or does not exist, and 255 everywhere for a row whose status
 *   is neither 0 nor 7.  A maximum matching is not unique: what is promised is that mate is a valid maximum matching of (N, E) and that
 *   the three entries give the same one (they are one source).  Every element of the given outputs is written, nothing else is.
 * mvae_smiles_kekule_rows / _corpus / _host: the inputs of mvae_smiles_scaffold_rows / _corpus / _host.  One thread per row;
 *   MVAE_KEKULE_LDS_BYTES = 73728 B (72 KiB) of LDS per 64-row block, so that two blocks fit a CU: the atom words (32 KiB), the closure
 *   pairs (8 KiB) and four byte arrays -- mate, parent, base, queue (8 KiB each).  Every loop is bounded by the 127 atoms a row can have.
 * Refused before anything is enqueued: what the scaffold entries refuse of these arguments (V > 64: MVAE_ERR_UNSUPPORTED; the rest
 *   MVAE_ERR_INVALID), and a NULL desc.
 */
#define MVAE_SMILES_KEKULE 7
#define MVAE_KEKULE_DESC 4
#define MVAE_KEKULE_LDS_BYTES 73728
int mvae_smiles_kekule_rows(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info /* [V] */,
                            const int32_t* chem_info /* [V] */, int eos_id, int32_t* status /* [B] */, int32_t* desc /* [B, 4] */,
                            uint8_t* mate /* [B, 128] or NULL */, void* stream);
int mvae_smiles_kekule_corpus(const uint8_t* tokens, const int64_t* offsets /* [N + 1] */, int64_t N, int V, const int32_t* tok_info /* [V] */,
                              const int32_t* chem_info /* [V] */, int32_t* status /* [N] */, int32_t* desc /* [N, 4] */,
                              uint8_t* mate /* [N, 128] or NULL */, void* stream);
int mvae_smiles_kekule_host(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info /* [V] */,
                            const int32_t* chem_info /* [V] */, int eos_id, int32_t* status /* [B] */, int32_t* desc /* [B, 4] */,
                            uint8_t* mate /* [B, 128] or NULL */);

/* ---------------------------------------------------------------------------------------------------------
 * SMILES rewrite (an addition: a fifth consumer of the "SMILES graph" walk above, and the first that writes a string).  A token row is
 * read into its graph and written back as another well-formed row that spells the same graph -- a randomised SMILES, the usual
 * augmentation for string models of molecules.  The spelling is a pure function of (row, seed, draw): there is no RNG state anywhere.
 * What this is NOT: no canonical SMILES (the priorities are a hash, not a refinement), no stereochemistry, not rdkit's
 *   MolToSmiles(doRandom=True): the set of spellings reached is this section's, and only "same graph under this library's walk" is claimed.
 * Graph.  The walk's graph with the fingerprint's recorder: atoms in string order, the order of the bond of every atom to its tree
 *   predecessor, the closure pairs (order 1), the ring mask.  h(a), the hydrogens of a bracket atom = its used valence minus the sum of
 *   its bond contributions (the orders of its tree bonds, 1 per closure).
 * Refusals.  A refused row is copied through unchanged (below) and its status says why:
 *   1 - 6  the walk's status, for a row the walk does not give 0;
 *   8  MVAE_SMILES_STEREO       the row has a token of class AT, or a bond token '/' or '\' (the ids of emit's stereo mask).  The walk
 *        ignores stereo: keeping the tokens would be wrong, dropping them would change the molecule silently;
 *   9  MVAE_SMILES_RING_MULTI   the traversal made a ring closure of a bond of order 2 or 3 (the grammar has no bond token before a digit);
 *   10 MVAE_SMILES_RING_DIGITS  no ring digit was free;
 *   11 MVAE_SMILES_DEPTH        more than 15 open branches;
 *   12 MVAE_SMILES_LONG         more than max_content content tokens;
 *   13 MVAE_SMILES_NO_TOKEN     the emit table has -1 for a token the output needs.
 *   (7 stays the kekule entries'.)  Precedence: the walk's status; then STEREO; then RING_MULTI (the whole traversal runs before anything
 *   is written); then whichever of 10 - 13 comes first as the tokens are written in order -- a "(" tests DEPTH before it is written,
 *   a token tests NO_TOKEN before LONG.
 * Priorities.  All arithmetic mod 2^32, mix the "Circular fingerprint" section's.  prio(a) = mix(mix(seed * 0x9E3779B1 + draw_b) ^
 *   (a * 0x85EBCA6B)) for atom a (string order) of row b; draw_b = draw[b] (uint32 [B]), or b when draw is NULL.  Atoms compare by
 *   (prio, atom number).
 * Traversal.  A depth-first search from the least atom.  At an atom its bonds other than the one to its search parent are taken in this
 *   order: the bonds of order 2 or 3 first, then by the other end's (prio, number) ascending.  An unvisited other end becomes a child (and is searched at
 *   once); a visited one with a smaller search index is an ancestor and the bond becomes a ring closure -- RING_MULTI if its order is not
 *   1; a visited one with a larger index is a descendant that has closed that bond already.  Multiple bonds first keeps them on the tree:
 *   RING_MULTI then needs one atom with two multiple bonds on a common cycle (C1=C=CCCC1 on some draws; never O=S1(=O)CCCC1 or C1=CC=CC=C1).
 * Emission, in pre-order of the search tree.  For each atom, in this order:
 *   the bond to its parent: '=' / '#' for a tree bond of order 2 / 3, nothing for order 1 (between aromatic atoms too: the walk reads
 *     "cc", "c-c" and "c:c" alike);
 *   the atom: unbracketed, its element token (lower case if aromatic; Cl, Br as head plus tail); a bracket atom as '[', the symbol, 'H' if
 *     h >= 1, the digit h if h >= 2, '+' / '-' for charge +1 / -1, ']'.  [N+1] becomes [N+]; [C] and [CH4] stay bracketed;
 *   the ring digits it closes (it is the descendant), by digit value 0 .. 9 ascending; they become free;
 *   the ring digits it opens (it is the ancestor), one per closure in ascending search index of the descendant: each the first of
 *     1 2 .. 9 0 that is neither open nor written at this atom already (the automaton refuses a digit twice on one atom); none: RING_DIGITS;
 *   its children in visiting order, every one but the last as '(' subtree ')', the last bare.  A '(' with 15 branches open: DEPTH.
 *   A token beyond max_content: LONG.
 * emit int32 [MVAE_REWRITE_EMIT = 48] (vocab.smiles_emit_table): one id per role, -1 where the vocabulary has no usable token --
 *   [0 .. 10] the first character of element e written upper case (H B C N O F P S C(l) B(r) I), [11 .. 21] lower case (b c n o p s only),
 *   22 'l', 23 'r', 24 '[', 25 ']', 26 'H', 27 '+', 28 '-', 29 '=', 30 '#', 31 '(', 32 ')', [33 .. 42] the digits 0 .. 9, 43 / 44 the low /
 *   high 32 bits of the stereo mask (bit i: id i is '@', '/' or '\'), the rest 0.
 * mvae_smiles_rewrite_rows (padded rows, <bos> in column 0, the inputs of mvae_smiles_kekule_rows):
 *   out int64 [B, T_out]: bos_id, the new tokens, eos_id, then pad_id.  A refused row: columns 0 .. k - 1 of x, k = the column of its first
 *     eos_id plus one (T without one), then pad_id.  A row longer than T_out is cut at T_out.
 *   out_len int32 [B]: tokens + 2, or k: the uncut length, so out_len[b] > T_out tells a cut row.  status int32 [B].
 * mvae_smiles_rewrite_corpus (rows int64 [B] of the CSR corpus, the end of a row acting as <eos>), one launch:
 *   tokens_out uint8 [B, stride]: batch member b's new tokens (a refused row: its own) from byte b * stride, zeros up to the next;
 *   offsets_out int64 [2 B + 1] = 0, len_0, stride, stride + len_1, 2 stride, ..., B stride: tokens_out as a CSR of 2 B rows whose even
 *     rows are the batch members and whose odd rows are the gaps, so mvae_moses_collate with rows = 0, 2, 4, .. collates it as it stands;
 *   err int32 [1] (optional, the caller zeroes it): raised with atomicMax to 1 by a refused row longer than stride, which is cut at
 *     stride, and to 2 by a row id outside [0, N), which gives an empty row with status 1.
 * Both take counts int32 [16] (optional, the caller zeroes it): counts[s] += the rows of status s, by integer atomic adds -- exact.
 * mvae_smiles_rewrite_host: _rows on host memory, the same source compiled for the CPU (no counts).
 * Every element of the given outputs is written, nothing else is; two runs are bit-identical.
 * One thread per row; MVAE_REWRITE_LDS_BYTES = 81920 B (80 KiB) of LDS per 64-row block, so that two blocks fit a CU: the atom words
 *   (32 KiB), the closure pairs, whose storage becomes the staged output row (8 KiB), the adjacency as <= 252 half-edge bytes (16 KiB)
 *   and three byte arrays -- CSR start, search index, search parent (8 KiB each).  No recursion and no stack: the search returns through
 *   the parent array.  Every loop is bounded by the 127 atoms and 252 half-edges a row can have.  The staged rows are stored by the
 *   whole wave over consecutive columns.
 * Refused before anything is enqueued: what the scaffold entries refuse of these arguments (V > 64: MVAE_ERR_UNSUPPORTED; the rest
 *   MVAE_ERR_INVALID), a NULL emit or output (counts, err and draw may be NULL), max_content outside [1, 127], T_out < 2, bos_id / pad_id
 *   outside [0, 65535], a NULL rows, B < 1, stride < max_content.
 */
#define MVAE_SMILES_STEREO 8
#define MVAE_SMILES_RING_MULTI 9
#define MVAE_SMILES_RING_DIGITS 10
#define MVAE_SMILES_DEPTH 11
#define MVAE_SMILES_LONG 12
#define MVAE_SMILES_NO_TOKEN 13
#define MVAE_REWRITE_EMIT 48
#define MVAE_REWRITE_LDS_BYTES 81920
int mvae_smiles_rewrite_rows(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info /* [V] */,
                             const int32_t* chem_info /* [V] */, const int32_t* emit /* [48] */, int bos_id, int eos_id, int pad_id,
                             uint32_t seed, const uint32_t* draw /* [B] or NULL */, int max_content, int T_out, int64_t* out /* [B, T_out] */,
                             int32_t* out_len /* [B] */, int32_t* status /* [B] */, int32_t* counts /* [16] or NULL */, void* stream);
int mvae_smiles_rewrite_corpus(const uint8_t* tokens, const int64_t* offsets /* [N + 1] */, int64_t N, const int64_t* rows /* [B] */, int B,
                               int V, const int32_t* tok_info /* [V] */, const int32_t* chem_info /* [V] */, const int32_t* emit /* [48] */,
                               uint32_t seed, const uint32_t* draw /* [B] or NULL */, int max_content, int stride,
                               uint8_t* tokens_out /* [B, stride] */, int64_t* offsets_out /* [2 B + 1] */, int32_t* status /* [B] */,
                               int32_t* counts /* [16] or NULL */, int32_t* err /* [1] or NULL */, void* stream);
int mvae_smiles_rewrite_host(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info /* [V] */,
                             const int32_t* chem_info /* [V] */, const int32_t* emit /* [48] */, int bos_id, int eos_id, int pad_id,
                             uint32_t seed, const uint32_t* draw /* [B] or NULL */, int max_content, int T_out, int64_t* out /* [B, T_out] */,
                             int32_t* out_len /* [B] */, int32_t* status /* [B] */);

/* ---------------------------------------------------------------------------------------------------------
 * SMILES canon (an addition: a sixth consumer of the "SMILES graph" walk above).  A token row is read into its graph and written back
 * as ONE spelling that is meant not to depend on how the row was spelled, so that rows can be compared as molecules by comparing tokens.
 * Graph, refusals, traversal, emission, the emit table and the output layouts are exactly the "SMILES rewrite" section's; only the
 * order of the atoms changes: atoms compare by canonical rank where that section says (prio, atom number).  There is no seed and no
 * draw, and no new status code; a refused row is copied through unchanged, as there.
 * First invariant.  Every atom gets the tuple (element -- its number in H B C N O F P S Cl Br I --, aromatic, charge, bracket flag,
 *   bracket hydrogens h(a) (0 for an unbracketed atom), degree, sum of its bond orders), compared left to right; rank(a) = the position
 *   of a's tuple among the distinct tuples.  The bracket flag is part of it: [CH4] and C stay different strings, as the rewrite keeps them.
 * Refinement.  key(a) = (rank(a), the multiset of (bond order, rank(b)) over the neighbours b of a, compared as an ascending sorted
 *   tuple); the new rank(a) = the position of key(a) among the distinct keys.  Rounds are repeated until one does not raise the number of
 *   classes (distinct ranks).  The comparison is exact: nothing is hashed.  Bond orders are the graph's: 1, 2, 3, a closure 1, a bond
 *   between aromatic atoms 1.
 * Ties.  While there are fewer classes than atoms: in the class of lowest rank that has more than one member, the member of lowest atom
 *   number (string order) keeps the rank and the others come just above it (every higher rank moves up by one); then refine again.
 * Bounds.  Every round of a refinement but its last adds a class, and so does every tie; n atoms have at most n classes, so there are at
 *   most n - 1 ties and class-adding rounds together, at most n refinements, and at most 2 n rounds in all.  The loops are bounded by that.
 * Search.  The root is the atom of rank 0; at an atom, bonds of order 2 or 3 first, then by the other end's rank; RING_MULTI and the
 *   other refusals keep the rewrite's precedence.
 * What is claimed.  Equal output rows (status 0) => equal graphs, always: the output spells the input's graph.  Equal graphs => equal
 *   output rows whenever, at every tie, the members of the chosen class are equivalent under a symmetry of the graph; that holds on the
 *   whole test corpus, cage and spiro rows included, where every choice at every tie is followed, and is NOT proved in general.
 *   A known instance where it fails: C1CCC(CC1)CCCCCC1CCCCC1 (1,5-dicyclohexylpentane).  The equitable partition ties ring atoms with
 *   chain atoms, following every choice at every tie reaches two strings, and the spelling depends on the order of the input.
 * What this is NOT: not rdkit's canonical SMILES.  No aromaticity perception (C1=CC=CC=C1 and c1ccccc1 stay two strings), no stereo
 *   (STEREO refuses such rows), [CH4] is not unbracketed.  (mvae_smiles_aromatize_*, "Aromatic normal form" below, is this spelling
 *   behind an aromaticity perception: there the two are one string.)
 * mvae_smiles_canon_rows / _corpus / _host take the arguments of mvae_smiles_rewrite_rows / _corpus / _host without seed and draw, and
 *   two more outputs, both optional (may be NULL):
 *   info int32 [B, 4] = atoms, classes after the first refinement, refinement rounds in all, ties broken -- for every row whose ranks
 *     were computed (the walk gave 0 and no stereo token: status 0 and 9 - 13), zeros otherwise;
 *   rank uint8 [B, 128]: rank[k] = the canonical rank of atom k (string order), a permutation of 0 .. atoms - 1; 0xFF beyond the atoms,
 *     and everywhere for a row whose ranks were not computed.
 *   Every element of the given outputs is written, nothing else is; two runs are bit-identical; the three entries are one source.
 * One thread per row; MVAE_CANON_LDS_BYTES = 81920 B (80 KiB) of LDS per 64-row block, the rewrite's block with nothing added, so that
 *   two blocks fit a CU: between the adjacency and the search the output row, the search index and the search parent are idle, and the
 *   ranks, the atoms sorted by rank and the new ranks live there.  Keys are recomputed from the ranks and the half-edges, never stored;
 *   only atoms of one class are compared.  The worst row is 127 atoms in a chain (126 rounds).
 * Refused before anything is enqueued: what the rewrite entries refuse of these arguments.
 */
#define MVAE_CANON_INFO 4
#define MVAE_CANON_LDS_BYTES 81920
int mvae_smiles_canon_rows(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info /* [V] */,
                           const int32_t* chem_info /* [V] */, const int32_t* emit /* [48] */, int bos_id, int eos_id, int pad_id,
                           int max_content, int T_out, int64_t* out /* [B, T_out] */, int32_t* out_len /* [B] */, int32_t* status /* [B] */,
                           int32_t* counts /* [16] or NULL */, int32_t* info /* [B, 4] or NULL */, uint8_t* rank /* [B, 128] or NULL */,
                           void* stream);
int mvae_smiles_canon_corpus(const uint8_t* tokens, const int64_t* offsets /* [N + 1] */, int64_t N, const int64_t* rows /* [B] */, int B,
                             int V, const int32_t* tok_info /* [V] */, const int32_t* chem_info /* [V] */, const int32_t* emit /* [48] */,
                             int max_content, int stride, uint8_t* tokens_out /* [B, stride] */, int64_t* offsets_out /* [2 B + 1] */,
                             int32_t* status /* [B] */, int32_t* counts /* [16] or NULL */, int32_t* err /* [1] or NULL */,
                             int32_t* info /* [B, 4] or NULL */, uint8_t* rank /* [B, 128] or NULL */, void* stream);
int mvae_smiles_canon_host(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info /* [V] */,
                           const int32_t* chem_info /* [V] */, const int32_t* emit /* [48] */, int bos_id, int eos_id, int pad_id,
                           int max_content, int T_out, int64_t* out /* [B, T_out] */, int32_t* out_len /* [B] */, int32_t* status /* [B] */,
                           int32_t* info /* [B, 4] or NULL */, uint8_t* rank /* [B, 128] or NULL */);

/* ---------------------------------------------------------------------------------------------------------
 * SMILES substructure (an addition: a seventh consumer of the "SMILES graph" walk above).  Does the molecule a token row spells contain
 * a given fragment?  The graph is the walk's, with the bond classes of "Circular fingerprint"; nothing is perceived and no toolkit is
 * matched: this is NOT SMARTS and NOT rdkit's HasSubstructMatch.
 * Query.  A SMILES fragment in the same vocabulary, a padded row like x (bos first), compiled once on the host into a table of
 *   MVAE_SUBSTRUCT_WORDS int32 words.  It has at most MVAE_SUBSTRUCT_QATOMS = 32 atoms; a launch takes at most MVAE_SUBSTRUCT_QUERIES =
 *   64 queries.  It must be a row the walk gives status 0 or 5 (AROMATIC: "an aromatic atom outside a ring" is the one rule that speaks
 *   about the whole molecule, not the fragment, so cC(=O)O and c[N+](=O)[O-] are queries).  Refused, with qstatus[q] = the reason and a
 *   table of zeros (a query without atoms, which no row contains): any other walk status (1 - 4, 6); else a stereo token '@' '/' '\'
 *   (MVAE_SMILES_STEREO); else more than 32 atoms (MVAE_SMILES_QUERY_ATOMS = 14, given by the compile entry alone).
 * Match.  Row t contains query q iff there is an injective map m from the query's atoms to the row's atoms with
 *   1. atoms: for every query atom i, element, aromatic flag and charge of i and m(i) are equal.  The bracket flag and hydrogen counts
 *      are not compared: [nH] matches any aromatic n.  [H] is an atom of element H and matches only an explicit [H];
 *   2. bonds: for every query bond (i, j), m(i) and m(j) are bonded with the same class -- 1, 2, 3, or 4 for a single bond between two
 *      aromatic atoms; ring-closure bonds count like any others.
 *   A monomorphism: the row may have more bonds among the matched atoms.
 * Search.  Fixed, so that the first match and the number of steps are defined.
 *   Prefilter: for each of the ten heavy elements B .. I, if the query has more atoms of it than the row, the result is a miss, 0 steps.
 *   Order: query atoms are placed in string order 0 .. nq - 1.  The candidates for atom 0 are the row's atoms in ascending order.  For
 *     atom i > 0 the anchor is its lowest-numbered query neighbour below i (the tree predecessor is one), and its candidates are the
 *     neighbours of m(anchor) in ascending atom number.
 *   Steps: one step is one candidate examined, whatever rejects it -- already used, atom mismatch, fewer neighbours than the query
 *     atom, or a missing or wrong-class bond to an earlier-placed query neighbour.  The first complete assignment ends the search; it is
 *     the lexicographically smallest embedding (m(0), m(1), ...).
 *   Budget: max_steps per (row, query), 1 .. MVAE_SUBSTRUCT_MAX_STEPS = 2^20.  A search that would examine step max_steps + 1 stops
 *     UNDECIDED, which is neither hit nor miss.  A search that ends within max_steps steps is decided.
 * Table of one query (int32 [MVAE_SUBSTRUCT_WORDS = 100]):
 *   word 0        nq, the atoms
 *   words 1 - 3   the atoms of element e = 1 .. 10, one byte each: e = 1 .. 4 in word 1, 5 .. 8 in word 2, 9 .. 10 in word 3
 *   words 4 + 3 i .. 6 + 3 i, for atom i:
 *     first word   bits 0-3 element, 4 aromatic, 5-6 charge + 1 (the key), 8-10 degree, 12-16 anchor, 20-22 the class of the bond to the
 *                  anchor, 24-26 the number of other neighbours below i (<= 5)
 *     second, third  those other neighbours in ascending order, one byte each from bit 0 of the second word: bits 0-4 the neighbour,
 *                  5-7 the class of the bond to it
 *   The search entries read a table as it is, with every index masked: a table that the compile entry did not write gives results
 *   without meaning and nothing worse.
 * mvae_smiles_substruct_compile_host: Q query rows xq [Q, Tq] into table [Q, 100] and qstatus [Q].  stereo_lo / stereo_hi: the mask of
 *   the stereo tokens' ids (words 43 / 44 of the rewrite's emit table).  Host only.
 * mvae_smiles_substruct_rows (padded rows) / _corpus (the CSR corpus, one launch, row b = corpus row b; an empty row is what the graph
 *   entry makes of it) / _host (the rows entry compiled for the CPU from the same source; counts is accumulated there too):
 *   status    int32 [B]              the walk's status, as the graph entries give it
 *   hit       int64 [B]              bit q set: the row contains query q (bit 63 is the sign bit)
 *   undecided int64 [B]              bit q set: the budget ran out on query q
 *   map       uint8 [B, 32] or NULL  the first embedding for the one query map_query; 0xFF beyond nq and where there is no hit
 *   steps     int32 [B, Q] or NULL   the steps examined per (row, query)
 *   counts    int32 [Q, 2] or NULL   += the rows that hit and the rows undecided, per query (integer atomics: one ballot and one add
 *                                    per wave and figure)
 *   A row of status != 0 gets zeros in hit, undecided and steps and 0xFF in map.  Every element of every given output is written
 *   (counts is added to), nothing else is; two runs are bit-identical.
 * One thread per row; MVAE_SUBSTRUCT_LDS_BYTES = 81920 B (80 KiB) of LDS per 64-row block, the rewrite's block with nothing added: the
 *   map and the cursors (32 bytes per lane each) and the current query's table (400 B per block) live where the adjacency's scratch
 *   arrays were.  A row's graph is built once and all Q queries run against it.
 * Refused before anything is enqueued.  MVAE_ERR_UNSUPPORTED: V > 64.  MVAE_ERR_INVALID: everything the graph entries refuse; Q outside
 *   1 .. 64; a NULL table, status, hit or undecided; map given with map_query outside [0, Q); max_steps outside 1 .. 2^20.
 */
#define MVAE_SUBSTRUCT_QATOMS 32
#define MVAE_SUBSTRUCT_QUERIES 64
#define MVAE_SUBSTRUCT_WORDS 100
#define MVAE_SUBSTRUCT_MAX_STEPS 1048576
#define MVAE_SUBSTRUCT_LDS_BYTES 81920
#define MVAE_SMILES_QUERY_ATOMS 14
int mvae_smiles_substruct_compile_host(int Q, int Tq, int V, const int64_t* xq, int64_t xq_ld, const int32_t* tok_info /* [V] */,
                                       const int32_t* chem_info /* [V] */, uint32_t stereo_lo, uint32_t stereo_hi, int eos_id,
                                       int32_t* table /* [Q, MVAE_SUBSTRUCT_WORDS] */, int32_t* qstatus /* [Q] */);
int mvae_smiles_substruct_rows(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info /* [V] */,
                               const int32_t* chem_info /* [V] */, int eos_id, int Q, const int32_t* table /* [Q, 100] */, int max_steps,
                               int map_query, int32_t* status /* [B] */, int64_t* hit /* [B] */, int64_t* undecided /* [B] */,
                               uint8_t* map /* [B, 32] or NULL */, int32_t* steps /* [B, Q] or NULL */, int32_t* counts /* [Q, 2] or NULL */,
                               void* stream);
int mvae_smiles_substruct_corpus(const uint8_t* tokens, const int64_t* offsets /* [N + 1] */, int64_t N, int V,
                                 const int32_t* tok_info /* [V] */, const int32_t* chem_info /* [V] */, int Q,
                                 const int32_t* table /* [Q, 100] */, int max_steps, int map_query, int32_t* status /* [N] */,
                                 int64_t* hit /* [N] */, int64_t* undecided /* [N] */, uint8_t* map /* [N, 32] or NULL */,
                                 int32_t* steps /* [N, Q] or NULL */, int32_t* counts /* [Q, 2] or NULL */, void* stream);
int mvae_smiles_substruct_host(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info /* [V] */,
                               const int32_t* chem_info /* [V] */, int eos_id, int Q, const int32_t* table /* [Q, 100] */, int max_steps,
                               int map_query, int32_t* status /* [B] */, int64_t* hit /* [B] */, int64_t* undecided /* [B] */,
                               uint8_t* map /* [B, 32] or NULL */, int32_t* steps /* [B, Q] or NULL */, int32_t* counts /* [Q, 2] or NULL */);

/* ---------------------------------------------------------------------------------------------------------
 * Scaffold SMILES (an addition: an eighth consumer of the "SMILES graph" walk above, and the third that writes a string).  The Murcko
 * scaffold of a token row as a token row: the scaffold graph G_S of the row, in the spelling of "SMILES canon", so that scaffolds can be
 * read, written to a file, passed on as substructure queries, and compared exactly by comparing tokens.
 * What this is NOT: not rdkit's MurckoScaffoldSmiles.  Nothing is sanitised, no aromaticity is perceived (C1=CC=CC=C1 and c1ccccc1 have
 *   two scaffolds), and there is no stereo: a row with a stereo token gets status STEREO and no scaffold.  There is no generic
 *   (all-carbon) framework mode.  (Rows put through mvae_smiles_aromatize_* first, "Aromatic normal form" below, have one.)
 * The scaffold graph G_S.  S = Core u Exo, exactly as "Murcko scaffold" defines them.  The atoms of G_S are the atoms of S, numbered in
 *   string order among themselves; its bonds are the row's bonds between two atoms of S, with their orders.
 * Hydrogens.  Every kept atom keeps its total valence, and the bonds it loses become hydrogens.
 *   h_row(a): the bracket H count of a bracket atom; for an unbracketed atom its implicit hydrogens by the rule of "SMILES graph".
 *   lost(a): the sum of the orders of a's bonds to atoms outside S (explicit [H] neighbours included).
 *   h_S(a) = h_row(a) + lost(a).
 *   A bracket atom stays a bracket atom, with H count h_S; element, aromatic flag and charge are kept.
 *   An unbracketed atom stays unbracketed iff the implicit-hydrogen rule, applied to its bond sum in G_S, gives exactly h_S; otherwise it
 *     becomes a bracket atom with H count h_S and charge 0.
 *   Cn1cccc1 -> c1cc[nH]c1; C[n+]1ccccc1 -> c1cc[nH+]cc1; C[N+]1(C)CCCC1 -> C1CC[NH2+]C1; O=C1CCCCC1C -> C1CCC(=O)CC1;
 *   N#Cc1ccc(Br)=c1 -> c1cc=[cH]c1; Clc1ccccc1 -> c1ccccc1; CP1(=O)CCCC1 -> C1CCP(=O)C1.
 *   Because valences are kept, the set N of "Kekulisation" and its matching are the same for the row and for its scaffold.
 * Spelling.  "SMILES canon" applied to G_S: its first invariant (with the bracket flag and the bracket hydrogens of G_S), its refinement,
 *   ties, search and emission, with nothing changed.
 * Canonicity is that section's claim, and carries its limit ("NOT proved in general").  One instance of the limit is known:
 *   C1CCC(CC1)CCCCCC1CCCCC1 (1,5-dicyclohexylpentane), where the equitable partition ties ring atoms with chain atoms, so that the
 *   members of the class chosen at a tie are not all equivalent under a symmetry: following every choice at every tie reaches two
 *   strings, and such a graph can be spelled two ways depending on the order of the input.  The test corpus has no such row.
 * Status.  0: the scaffold was written.  1 - 6: the walk's refusals.  8 - 13: the rewrite's refusals, with the rewrite's precedence, where
 *   STEREO is decided before S and 9 - 13 speak of the scaffold's spelling (LONG: the scaffold has more than max_content tokens).
 *   14 MVAE_SMILES_NO_RING: a row the walk gives 0, without a stereo token, that has no ring (S is empty); decided after STEREO and
 *   before the search.  (As a number, 14 is also the compile entry's MVAE_SMILES_QUERY_ATOMS; no entry gives both.)
 * mvae_smiles_scaffold_smiles_rows / _corpus / _host take the arguments of mvae_smiles_canon_rows / _corpus / _host without rank, and
 *   write their outputs in the same layouts, with one difference: a row whose status is not 0 gets the EMPTY row, never a copy of the
 *   input -- a molecule is not its own scaffold.  _rows / _host: bos_id, eos_id, then pad_id, and out_len = 2; _corpus: a slice of length
 *   0, and err is raised only by a row id outside [0, N) (to 2).  counts int32 [16] has room for status 14.
 *   info int32 [B, MVAE_SCAFFOLD_SMILES_INFO = 4] (optional, may be NULL) = |S|, the bonds of G_S, the atoms that became bracket atoms,
 *     the sum of lost(a) over S -- for status 0 and 9 - 13, zeros otherwise.
 *   Every element of every given output is written, nothing else is; two runs are bit-identical; the three entries are one source.
 * One thread per row; MVAE_SCAFFOLD_SMILES_LDS_BYTES = 81920 B (80 KiB) of LDS per 64-row block, the rewrite's block with nothing
 *   added: S is two 64-bit masks in registers, the atom words and the closure pairs are cut down to S in place (the new number of an
 *   atom is the count of the members of S below it), and the adjacency, the ranks and the search run on the cut arrays as they do in
 *   the canon entries.  No recursion; every loop is bounded by the 127 atoms a row can have.
 * Refused before anything is enqueued: exactly what the canon entries refuse of these arguments.
 */
#define MVAE_SMILES_NO_RING 14
#define MVAE_SCAFFOLD_SMILES_INFO 4
#define MVAE_SCAFFOLD_SMILES_LDS_BYTES 81920
int mvae_smiles_scaffold_smiles_rows(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info /* [V] */,
                                     const int32_t* chem_info /* [V] */, const int32_t* emit /* [48] */, int bos_id, int eos_id, int pad_id,
                                     int max_content, int T_out, int64_t* out /* [B, T_out] */, int32_t* out_len /* [B] */,
                                     int32_t* status /* [B] */, int32_t* counts /* [16] or NULL */, int32_t* info /* [B, 4] or NULL */,
                                     void* stream);
int mvae_smiles_scaffold_smiles_corpus(const uint8_t* tokens, const int64_t* offsets /* [N + 1] */, int64_t N, const int64_t* rows /* [B] */,
                                       int B, int V, const int32_t* tok_info /* [V] */, const int32_t* chem_info /* [V] */,
                                       const int32_t* emit /* [48] */, int max_content, int stride, uint8_t* tokens_out /* [B, stride] */,
                                       int64_t* offsets_out /* [2 B + 1] */, int32_t* status /* [B] */, int32_t* counts /* [16] or NULL */,
                                       int32_t* err /* [1] or NULL */, int32_t* info /* [B, 4] or NULL */, void* stream);
int mvae_smiles_scaffold_smiles_host(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info /* [V] */,
                                     const int32_t* chem_info /* [V] */, const int32_t* emit /* [48] */, int bos_id, int eos_id, int pad_id,
                                     int max_content, int T_out, int64_t* out /* [B, T_out] */, int32_t* out_len /* [B] */,
                                     int32_t* status /* [B] */, int32_t* info /* [B, 4] or NULL */);

/* ---------------------------------------------------------------------------------------------------------
 * Fragments (an addition: a ninth consumer of the "SMILES graph" walk above, and the fourth family that writes a string).  A row cut
 * into pieces at its ring substituent bonds and its acyl-heteroatom bonds; every piece gets the graph key of "Graph key" and can be
 * written as a token row.  The fragment histogram of a set of rows is what the MOSES Frag figure compares.
 * What this is NOT: it is this library's own rule -- not BRICS, not RECAP, not rdkit's fragmenters --, and agreement with any toolkit is
 *   neither tested nor claimed.  No dummy atoms mark the cut ends.  It is defined on the graph exactly as the walk builds it: explicit [H]
 *   are atoms, ring-closure bonds are order 1, nothing is kekulised or sanitised, no aromaticity is perceived, stereo carries nothing.
 * Where a row is cut.  G is the walk's graph of a valence-consistent row, deg(a) the number of bonds of atom a in G.  A bond a - b is
 *   cut iff all of these hold:
 *   1. its recorded order is 1 (a closure is a ring bond and is never cut);
 *   2. it is not a ring bond ("Murcko scaffold"): it is a bridge, and every bridge is a tree bond;
 *   3. deg(a) >= 2 and deg(b) >= 2: a terminal atom -- a methyl, a halogen, a hydroxyl -- is never cut off;
 *   4. at least one of
 *      R (ring rule): a or b is a ring atom;
 *      A (acyl rule): one end is a non-ring atom with a double bond to an O or S atom of degree 1, and the other end is an N, O or S
 *        atom (amide, ester, carbamate, urea, sulfonamide, phosphate ester).
 * What comes out.  The fragments are the connected components of G without the cut bonds, numbered by their lowest atom in string order;
 *   a row with c cut bonds has c + 1 of them.
 *   Fragment key: the "Graph key" of the fragment's atom set U with its induced bonds, exactly as the scaffold key is made:
 *     w_U(a) = elem | arom << 4 | (charge + 1) << 5 | in_ring << 7 | deg_U(a) << 8, no used valence; ring membership and ring bonds are
 *     those of the whole row.  No new hash.  A benzene ring cut out of any row has the scaffold key of benzene.
 *   Fragment SMILES: the row's graph cut down to U, every lost bond turned into a hydrogen of the atom that lost it as "Scaffold SMILES"
 *     defines (h_U = h_row + lost), in the spelling of "SMILES canon", with that section's claim and limit.
 *   CC(=O)Oc1ccccc1C(=O)O: 3 cuts (C-O of the ester by rule A alone), 4 fragments CC=O, O, c1ccccc1, O=CO.  Cc1ccccc1, CCOCC: no cut.
 *   c1ccccc1c1ccccc1: 1 cut, c1ccccc1 twice.  CC(=O)NC: 1 cut by rule A alone, CC=O and CN.  CCn1cccc1: 1 cut, CC and c1cc[nH]c1.
 * mvae_smiles_fragment_rows / _corpus / _host: the inputs of mvae_smiles_scaffold_rows / _corpus / _host.  Outputs, per row, with
 *   F = MVAE_FRAGMENT_MAX = 16: status int32 [B]; mask int64 [B, F, 2] (optional, may be NULL): bit a of word a >> 6 of slot f = atom a is
 *   in fragment f; desc int32 [B, MVAE_FRAGMENT_DESC = 4] = fragments, cut bonds, cut bonds that rule A alone cuts, atoms of the largest
 *   fragment; key int64 [B, F] = the fragment keys, 0 in the unused slots.  Every element of the given outputs is written, nothing else is.
 *   Status: 0 - 6 as the graph entries give it, and a row with status other than 0 gets zeros everywhere -- except
 *   15 MVAE_SMILES_FRAG_MANY: a row the walk gives 0 that has more than F fragments.  Its mask and key are all zeros and its desc holds
 *   the true four counts: nothing is silently truncated.
 *   One thread per row; MVAE_FRAGMENT_LDS_BYTES = 81920 B (80 KiB) of LDS per 64-row block, the scaffold entry's arrays with nothing
 *   added.  The refinement rounds run once per row over all atoms with the cut bonds left out -- no bond joins two fragments, so every
 *   atom ends with the id a run over its fragment alone would give it -- and one walk along each fragment's atoms sums them into its key.
 *   Refused before anything is enqueued: what the scaffold entries refuse.
 * mvae_smiles_fragment_smiles_rows / _corpus / _host take the arguments of mvae_smiles_scaffold_smiles_rows / _corpus / _host with
 *   `int frag` in front of info, and write fragment number frag of every row in the same layouts.  A row whose status is not 0 gets the
 *   EMPTY row, never a copy.  Status: 0: written.  1 - 6: the walk's refusals.  8 - 13: the rewrite's, with STEREO decided before the
 *   cuts and 9 - 13 speaking of the fragment's spelling.  16 MVAE_SMILES_NO_FRAGMENT: a row the walk gives 0, without a stereo token, with
 *   frag or fewer fragments.  There is no upper limit on frag here: a FRAG_MANY row has its 17th fragment written.  counts, where given,
 *   is int32 [MVAE_FRAGMENT_SMILES_COUNTS = 32]: slot 16 counts NO_FRAGMENT (the writer families count status & 31; the others never
 *   give a status above 14, so their int32 [16] stands).  info int32 [B, MVAE_FRAGMENT_SMILES_INFO = 4] (optional) = atoms and bonds of
 *   the fragment, atoms that became bracket atoms, the sum of lost(a) -- for status 0 and 9 - 13, zeros otherwise.
 *   MVAE_FRAGMENT_SMILES_LDS_BYTES = 81920 B per 64-row block, the rewrite's block with nothing added; the cut set and the labels are
 *   the code of the keys entry.  Refused before anything is enqueued: what the scaffold SMILES entries refuse, and frag < 0.
 */
#define MVAE_FRAGMENT_MAX 16
#define MVAE_FRAGMENT_DESC 4
#define MVAE_FRAGMENT_LDS_BYTES 81920
#define MVAE_SMILES_FRAG_MANY 15
#define MVAE_SMILES_NO_FRAGMENT 16
#define MVAE_FRAGMENT_SMILES_INFO 4
#define MVAE_FRAGMENT_SMILES_COUNTS 32
#define MVAE_FRAGMENT_SMILES_LDS_BYTES 81920
int mvae_smiles_fragment_rows(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info /* [V] */,
                              const int32_t* chem_info /* [V] */, int eos_id, int32_t* status /* [B] */, int64_t* mask /* [B, 16, 2] or NULL */,
                              int32_t* desc /* [B, 4] */, int64_t* key /* [B, 16] */, void* stream);
int mvae_smiles_fragment_corpus(const uint8_t* tokens, const int64_t* offsets /* [N + 1] */, int64_t N, int V, const int32_t* tok_info /* [V] */,
                                const int32_t* chem_info /* [V] */, int32_t* status /* [N] */, int64_t* mask /* [N, 16, 2] or NULL */,
                                int32_t* desc /* [N, 4] */, int64_t* key /* [N, 16] */, void* stream);
int mvae_smiles_fragment_host(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info /* [V] */,
                              const int32_t* chem_info /* [V] */, int eos_id, int32_t* status /* [B] */, int64_t* mask /* [B, 16, 2] or NULL */,
                              int32_t* desc /* [B, 4] */, int64_t* key /* [B, 16] */);
int mvae_smiles_fragment_smiles_rows(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info /* [V] */,
                                     const int32_t* chem_info /* [V] */, const int32_t* emit /* [48] */, int bos_id, int eos_id, int pad_id,
                                     int max_content, int T_out, int64_t* out /* [B, T_out] */, int32_t* out_len /* [B] */,
                                     int32_t* status /* [B] */, int32_t* counts /* [32] or NULL */, int frag, int32_t* info /* [B, 4] or NULL */,
                                     void* stream);
int mvae_smiles_fragment_smiles_corpus(const uint8_t* tokens, const int64_t* offsets /* [N + 1] */, int64_t N, const int64_t* rows /* [B] */,
                                       int B, int V, const int32_t* tok_info /* [V] */, const int32_t* chem_info /* [V] */,
                                       const int32_t* emit /* [48] */, int max_content, int stride, uint8_t* tokens_out /* [B, stride] */,
                                       int64_t* offsets_out /* [2 B + 1] */, int32_t* status /* [B] */, int32_t* counts /* [32] or NULL */,
                                       int32_t* err /* [1] or NULL */, int frag, int32_t* info /* [B, 4] or NULL */, void* stream);
int mvae_smiles_fragment_smiles_host(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info /* [V] */,
                                     const int32_t* chem_info /* [V] */, const int32_t* emit /* [48] */, int bos_id, int eos_id, int pad_id,
                                     int max_content, int T_out, int64_t* out /* [B, T_out] */, int32_t* out_len /* [B] */,
                                     int32_t* status /* [B] */, int frag, int32_t* info /* [B, 4] or NULL */);

/* ---------------------------------------------------------------------------------------------------------
 * Aromatic normal form (an addition: a tenth consumer of the "SMILES graph" walk above, and the fifth family that writes a string).  A
 * token row is read into its graph, aromaticity is PERCEIVED on that graph by the rule below, and the row is written back in the
 * spelling of "SMILES canon" of the perceived graph: C1=CC=CC=C1, c1ccccc1 and every respelling of either come out as one token row.
 * What this is NOT: the rule is this library's own.  It is not rdkit's aromaticity model and the output is not rdkit's canonical SMILES;
 *   agreement with a toolkit is neither tested nor claimed.  There are no envelope cycles, so azulene stays Kekule (and azulene written
 *   in lower case is refused).  There are no rings of 3, 4, 8 or more atoms.  There is no P, B, Se.  There is no stereo: a row with a
 *   stereo token gets status STEREO.  The caveat of "SMILES canon" about ties ("NOT proved in general") carries over.
 * Kekule graph of a row.  The walk's graph, in which every atom of the set N of "Kekulisation" has one more ring double bond; which
 *   bond that is belongs to the matching, and nothing below depends on it.  U(a) is the used valence (bonds and bracket hydrogens).
 *   K(a) = U(a) + [a in N] + the implicit hydrogens of an unbracketed atom ("SMILES graph"): the true valence, hydrogens included.
 *   dbl(a) = the bonds of order 2 of a, plus one for a in N.  A row with lower-case atoms must kekulise ((N, E) has a perfect matching),
 *   otherwise its status is MVAE_SMILES_KEKULE, as the kekule entries give it.
 * Electrons.  An atom is a candidate iff it is a ring member and one of three cases holds:
 *   e = 1: dbl(a) = 1, no triple bond, the double bond is a ring bond (for an atom of N by construction), K(a) <= 4, and (element,
 *          charge) is C0, N0, N+, O+ or S+.  K <= 4 leaves out N and S+ of valence 5, so that a candidate has at most three bonds.
 *   e = 0: C0 with dbl(a) = 1 whose double bond is a non-ring bond to O, S or N: c(=O), C(=O).
 *   e = 2: dbl(a) = 0 and N0 with K = 3, O0 or S0 with K = 2, N- with K = 2, or C- with K = 3.
 *   Everything else is no candidate: sp3 atoms, B, P, an exocyclic C=C, S(=O), cations without a double bond.
 * Aromatic cycles.  Every simple cycle of 5, 6 or 7 atoms, all of them candidates (its bonds are ring bonds, being on a cycle), is
 *   aromatic iff the sum of e over its atoms is 2 (mod 4).  An atom is aromatic iff it lies on an aromatic cycle: a function of the
 *   graph alone, independent of the atom numbering and of which Kekule structure was written.  The cycles are enumerated by a path
 *   search from every start atom over candidate neighbours numbered above it, to 7 atoms: a candidate has at most 3 neighbours, so a
 *   start costs a few hundred steps at most, and no budget is needed.
 * Refusal.  17 MVAE_SMILES_NOT_AROMATIC: a row the walk accepts, without a stereo token, that kekulises, in which some lower-case atom
 *   is not aromatic by the rule: c1ccc1, c1ccccccc1, O=c1ccc(=O)cc1, c1cc2cccccc2c1, c1ccpcc1.  Precedence: the walk's status, STEREO
 *   (8), KEKULE (7), NOT_AROMATIC (17), the writer's 9 - 13.  A refused row is copied through unchanged, as the rewrite copies one.
 * Output graph.  The aromatic atoms get the aromatic flag, whatever case they were written in.  Every bond between two aromatic atoms
 *   gets order 1, and a former double bond lowers the used valence of both its ends by one.  Every atom keeps its true hydrogen count:
 *   a bracket atom stays a bracket atom (as in canon); an unbracketed atom stays unbracketed iff the implicit-hydrogen rule of "SMILES
 *   graph" on its new flag and new bond sum gives that count, and otherwise becomes a bracket atom with it: N1C=CC=C1 -> c1cc[nH]c1.
 *   Then the ranks and the writer of "SMILES canon" run on that graph unchanged.
 *   C1=CC=CC=C1 -> c1ccccc1; O=C1C=CC=CN1 -> O=c1cccc[nH]1; C1C=CC2=CC=CC=C12 -> C1=Cc2ccccc2C1 (the five-ring double bond stays);
 *   O=C1C=CC(=O)C=C1, C1=CC=CC=CC=C1, C1=CC=C1 and azulene C1=CC2=CC=CC=CC2=C1 have no aromatic atom and come out as canon writes them.
 * mvae_smiles_aromatize_rows / _corpus / _host take the arguments of mvae_smiles_canon_rows / _corpus / _host with arom in the place
 *   of rank, and write out / out_len / status (tokens_out / offsets_out / status / err) in the same layouts.  counts, where given, is
 *   int32 [MVAE_AROMATIZE_COUNTS = 32], the histogram of the statuses (17 must fit).
 *   info int32 [B, MVAE_AROMATIZE_INFO = 4] (optional, may be NULL) = atoms, aromatic atoms in the output, atoms written in upper case
 *     that came out aromatic, bonds of order 2 that became aromatic -- for status 0 and 9 - 13, zeros for a row whose output graph was
 *     not made (1 - 8, 17, a corpus id outside [0, N)).
 *   arom uint8 [B, 128] (optional, may be NULL) = 1 / 0 per atom in the string order of the input, 0xFF beyond the atoms, and 0xFF
 *     everywhere where info is zeros.
 *   Every element of every given output is written, nothing else is; two runs are bit-identical; the three entries are one source.
 * One thread per row; MVAE_AROMATIZE_LDS_BYTES = 81920 B (80 KiB) of LDS per 64-row block, the rewrite's block with nothing added:
 *   the matching's four byte arrays are the two halves of the half-edge list and two of the writer's byte arrays, which the adjacency
 *   fills only afterwards; the candidate neighbours (<= 3 per atom) stand in the three byte arrays; candidates, electrons and aromatic
 *   atoms are 64-bit masks in registers, the search path is one 64-bit register.  No recursion, no private array.
 * Refused before anything is enqueued: exactly what the canon entries refuse of these arguments.
 */
#define MVAE_SMILES_NOT_AROMATIC 17
#define MVAE_AROMATIZE_INFO 4
#define MVAE_AROMATIZE_COUNTS 32
#define MVAE_AROMATIZE_LDS_BYTES 81920
int mvae_smiles_aromatize_rows(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info /* [V] */,
                               const int32_t* chem_info /* [V] */, const int32_t* emit /* [48] */, int bos_id, int eos_id, int pad_id,
                               int max_content, int T_out, int64_t* out /* [B, T_out] */, int32_t* out_len /* [B] */,
                               int32_t* status /* [B] */, int32_t* counts /* [32] or NULL */, int32_t* info /* [B, 4] or NULL */,
                               uint8_t* arom /* [B, 128] or NULL */, void* stream);
int mvae_smiles_aromatize_corpus(const uint8_t* tokens, const int64_t* offsets /* [N + 1] */, int64_t N, const int64_t* rows /* [B] */,
                                 int B, int V, const int32_t* tok_info /* [V] */, const int32_t* chem_info /* [V] */,
                                 const int32_t* emit /* [48] */, int max_content, int stride, uint8_t* tokens_out /* [B, stride] */,
                                 int64_t* offsets_out /* [2 B + 1] */, int32_t* status /* [B] */, int32_t* counts /* [32] or NULL */,
                                 int32_t* err /* [1] or NULL */, int32_t* info /* [B, 4] or NULL */, uint8_t* arom /* [B, 128] or NULL */,
                                 void* stream);
int mvae_smiles_aromatize_host(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info /* [V] */,
                               const int32_t* chem_info /* [V] */, const int32_t* emit /* [48] */, int bos_id, int eos_id, int pad_id,
                               int max_content, int T_out, int64_t* out /* [B, T_out] */, int32_t* out_len /* [B] */,
                               int32_t* status /* [B] */, int32_t* info /* [B, 4] or NULL */, uint8_t* arom /* [B, 128] or NULL */);

/* ---------------------------------------------------------------------------------------------------------
 * SELFIES (an addition: decoding is an eleventh producer of the "SMILES graph" walk's graph and the sixth family that writes a string;
 * encoding is the seventh).  mvae_selfies_decode_* turn rows of SELFIES tokens into the canonical Kekule SMILES rows of "SMILES canon";
 * mvae_selfies_encode_* turn SMILES rows into SELFIES rows.
 * What this is NOT: the derivation below is this library's own, stated here in full.  The symbol spelling and the derivation follow
 *   SELFIES 2.x so that strings interchange in the ordinary case, but this is NOT the selfies package's decoder or encoder: agreement
 *   with the package is neither tested nor claimed.  No stereo, no isotopes, no elements beyond the eleven of "SMILES graph", charges in
 *   {-1, 0, +1}, at most 127 symbols and 127 atoms per row.
 * Symbols.  A SELFIES vocabulary maps token ids to symbols.  The kernels see one int32 [V] info table; a word holds
 *     bits 0-2   the kind: 0 other, 1 atom, 2 branch, 3 ring, 4 nop, 5 <eos>
 *     bits 3-4   beta, the requested bond order 1 - 3: [=X] is 2, [#X] is 3
 *     atom:      bits 5-8 the element (index into H B C N O F P S Cl Br I), 9-10 the charge + 1, 11 bracket atom, 12-14 stated hydrogens 0 - 4
 *     branch / ring:  bits 16-17 L, the number of index symbols that follow, 1 - 3
 *     bits 20-23 the index value 0 - 15 of the symbol read as a digit
 *   Atom symbols are spelled [bE], [bEHn], [bE+1], [bE-1], [bEHn+1], [bEHn-1] with b one of "", "=", "#": [C], [=N], [NH1], [=N+1], [O-1],
 *   [NH2+1].  A symbol with neither hydrogens nor charge is written as an unbracketed atom ([H] excepted); every other atom symbol is
 *   written as a bracket atom with exactly the stated hydrogens.  Index values: [C] 0, [Ring1] 1, [Ring2] 2, [Branch1] 3, [=Branch1] 4,
 *   [#Branch1] 5, [Branch2] 6, [=Branch2] 7, [#Branch2] 8, [O] 9, [N] 10, [=N] 11, [=C] 12, [#C] 13, [S] 14, [P] 15; every other symbol,
 *   and a symbol missing because the row or the enclosing branch ended, reads as 0.  An index of L symbols is read in base 16, most
 *   significant first.
 * Capacity.  cap(atom) = the largest valence of (element, charge) in "SMILES graph" minus the stated hydrogens; neutral I has 1 minus
 *   them.  A pair without an entry is no symbol, and neither is one whose capacity is below 1 (it could not be bonded to anything).
 *   Every capacity is at most the walk's largest valence, so every decoded row is valence-consistent under the walk by construction.
 * Derivation (decode).  The state: s, the bonds the previous atom can still make (0 before the first atom); prev, the atom the chain
 *   hangs from; a list of deferred ring bonds; a stack of (resume state, root atom, end of the branch).  Symbols in order:
 *   atom (beta, cap)   o = 0 if s == 0 (the first atom only), else min(beta, s, cap).  The atom is added with predecessor prev and bond
 *                      order o; prev = it, s = cap - o.  If s is 0 the chain ends: the symbols left in the current branch are consumed
 *                      without effect, at top level the rest of the row.
 *   branch (beta, L)   if s <= 1 the symbol is skipped and its index symbols are read as ordinary symbols.  Else b = min(s - 1, beta), Q
 *                      is read from the next L symbols, the next Q + 1 symbols (or what the enclosing branch has left) are derived with
 *                      start state b from root prev, and the chain resumes at the same prev with s - b.
 *   ring (beta, L)     if s == 0 it is skipped.  Else o = min(beta, s), Q is read, (l = max(0, prev - (Q + 1)), r = prev, o) is
 *                      recorded, s -= o, and if s is 0 the chain ends as above.
 *   nop                nothing.   <eos>, or the row end for a corpus row, ends the row.
 *   Any other token (<bos>, <pad>, <unk>, an id >= V) anywhere in the content, consumed or not, gives status 1 with its column in info,
 *   and so does a 128th symbol.  A row that adds no atom is status 1.
 *   After the last symbol the recorded ring bonds are applied in order: skip if l == r; o = min(o, cap(l) - bondsum(l), cap(r) -
 *   bondsum(r)) at that moment, skip if 0; if l and r are bonded already, by a tree bond or an earlier ring bond, that bond is raised by
 *   min(o, 3 - its order); else the ring bond is added.  A bracket atom has its stated hydrogens and unused capacity stays unused; an
 *   unbracketed atom gets the implicit hydrogens of "SMILES graph" on its bond sum.  The molecule a SELFIES row denotes is, by
 *   definition, the graph of the SMILES row written.
 * Into the writer.  The writer keeps ring closures as single bonds, so a ring bond of order >= 2 between l < r is made a tree bond: if
 *   r's tree bond is single and l does not hang below r, r's predecessor becomes l with the ring bond's order and (old predecessor, r)
 *   becomes the single closure; otherwise the same is tried at l; otherwise the row is MVAE_SMILES_RING_MULTI (9).  Then the adjacency,
 *   the ranks and the writer of "SMILES canon" run unchanged.  Statuses: 0, 1, and the writer's 9 - 13; 2 - 8 never occur.  A row that
 *   is not written gives the EMPTY row (<bos> <eos>; a corpus row of length 0), never a copy: its source is another language.
 * Encode.  rew::read (statuses 1 - 6, 8); with aromatic atoms the matching of "Kekulisation" (7 without a perfect one), the bonds (a,
 *   mate[a]) become double and the flags are dropped; a bracket atom gives the symbol with its hydrogens and charge, an unbracketed atom
 *   the plain one; an atom whose bonds exceed the capacity of its symbol is MVAE_SELFIES_CAPACITY (18): hypervalent iodine.  The atoms
 *   are emitted in increasing number, the SMILES string order.  For atom k: if k is a child of its predecessor but not the last one,
 *   [bBranchL] with b its bond order, Q = size(k) - 1 and the smallest L that holds it; then its atom symbol with its bond order; then
 *   for every ring closure whose later end is k, in increasing earlier end l, [RingL] or, for a closure that is double after
 *   kekulisation, [=RingL], with Q = k - l - 1.  size(k) = the symbols of k's subtree.  A symbol the vocabulary lacks (emit table entry
 *   -1), a bracket atom with neither hydrogens nor charge ([C]: its symbol would be read as the plain atom), or one with more than four
 *   hydrogens, is 13; output longer
 *   than max_content is 12.  The derivation of an encoded row skips no branch and ends no chain early.
 * The emit table of the encode side, int32 [MVAE_SELFIES_EMIT = 529], role -> id, -1 = missing: atom symbols at (((beta - 1) * 11 +
 *   element) * 3 + charge + 1) * 5 + hydrogens; [bBranchL] at 495 + (beta - 1) * 3 + L - 1; [bRingL] at 504 + the same; the symbol of
 *   index value v at 513 + v.
 * Entries.  Layouts of out / out_len / status, tokens_out / offsets_out / err and counts (int32 [MVAE_SELFIES_COUNTS = 32]) as in
 *   mvae_smiles_canon_*.  decode: V and sinfo describe the SELFIES vocabulary (its <eos> is the word of kind 5), emit is the SMILES
 *   emit table, bos_id / eos_id / pad_id are the SMILES ids written.  info int32 [B, 4] (may be NULL) = atoms, ring bonds kept, ring
 *   bonds re-parented, the column of the token behind status 1 (else -1).  encode: V, tok_info, chem_info, emit and eos_in describe the
 *   SMILES rows read, semit is the SELFIES emit table, bos_id / eos_id / pad_id are the SELFIES ids written.  info = atoms, branch
 *   symbols, ring symbols, the atom behind status 18 (else -1).  A corpus id outside [0, N) gives status 1, err 2 and info 0 0 0 -1.
 *   Every element of every given output is written; two runs are bit-identical; the three entries of a direction are one source.
 * One thread per row; MVAE_SELFIES_LDS_BYTES = 81920 B of LDS per 64-row block, the rewrite's block with nothing added.
 * Refused before anything is enqueued.  MVAE_ERR_UNSUPPORTED: V > 64.  MVAE_ERR_INVALID: a NULL pointer other than counts, err, info;
 *   V, B, T or N < 1; x_ld < T; max_content outside [1, 127]; T_out < 2; stride < max_content; an output id outside [0, 255]; eos_in
 *   outside [0, V).
 */
#define MVAE_SELFIES_CAPACITY 18
#define MVAE_SELFIES_EMIT 529
#define MVAE_SELFIES_COUNTS 32
#define MVAE_SELFIES_LDS_BYTES 81920
int mvae_selfies_decode_rows(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* sinfo /* [V] */, const int32_t* emit /* [48] */,
                             int bos_id, int eos_id, int pad_id, int max_content, int T_out, int64_t* out /* [B, T_out] */,
                             int32_t* out_len /* [B] */, int32_t* status /* [B] */, int32_t* counts /* [32] or NULL */,
                             int32_t* info /* [B, 4] or NULL */, void* stream);
int mvae_selfies_decode_corpus(const uint8_t* tokens, const int64_t* offsets /* [N + 1] */, int64_t N, const int64_t* rows /* [B] */, int B,
                               int V, const int32_t* sinfo /* [V] */, const int32_t* emit /* [48] */, int max_content, int stride,
                               uint8_t* tokens_out /* [B, stride] */, int64_t* offsets_out /* [2 B + 1] */, int32_t* status /* [B] */,
                               int32_t* counts /* [32] or NULL */, int32_t* err /* [1] or NULL */, int32_t* info /* [B, 4] or NULL */,
                               void* stream);
int mvae_selfies_decode_host(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* sinfo /* [V] */, const int32_t* emit /* [48] */,
                             int bos_id, int eos_id, int pad_id, int max_content, int T_out, int64_t* out /* [B, T_out] */,
                             int32_t* out_len /* [B] */, int32_t* status /* [B] */, int32_t* info /* [B, 4] or NULL */);
int mvae_selfies_encode_rows(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info /* [V] */,
                             const int32_t* chem_info /* [V] */, const int32_t* emit /* [48] */, int eos_in, const int32_t* semit /* [529] */,
                             int bos_id, int eos_id, int pad_id, int max_content, int T_out, int64_t* out /* [B, T_out] */,
                             int32_t* out_len /* [B] */, int32_t* status /* [B] */, int32_t* counts /* [32] or NULL */,
                             int32_t* info /* [B, 4] or NULL */, void* stream);
int mvae_selfies_encode_corpus(const uint8_t* tokens, const int64_t* offsets /* [N + 1] */, int64_t N, const int64_t* rows /* [B] */, int B,
                               int V, const int32_t* tok_info /* [V] */, const int32_t* chem_info /* [V] */, const int32_t* emit /* [48] */,
                               const int32_t* semit /* [529] */, int max_content, int stride, uint8_t* tokens_out /* [B, stride] */,
                               int64_t* offsets_out /* [2 B + 1] */, int32_t* status /* [B] */, int32_t* counts /* [32] or NULL */,
                               int32_t* err /* [1] or NULL */, int32_t* info /* [B, 4] or NULL */, void* stream);
int mvae_selfies_encode_host(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info /* [V] */,
                             const int32_t* chem_info /* [V] */, const int32_t* emit /* [48] */, int eos_in, const int32_t* semit /* [529] */,
                             int bos_id, int eos_id, int pad_id, int max_content, int T_out, int64_t* out /* [B, T_out] */,
                             int32_t* out_len /* [B] */, int32_t* status /* [B] */, int32_t* info /* [B, 4] or NULL */);

/* ---------------------------------------------------------------------------------------------------------
 * Tanimoto similarity of fingerprints (an addition: the structure-aware counterpart of mvae_latent_knn and mvae_edit_knn).  Fingerprints
 * are dense rows of MVAE_FP_WORDS int64 words, 16-byte aligned (else MVAE_ERR_INVALID); any 1024-bit rows will do.
 * Similarity.  T(a, b) = c / (p_a + p_b - c), with p the popcounts and c the popcount of a AND b; T is 0 when the union is empty.  T is
 *   ONE correctly rounded f32 division of the two integers.  Numerators and denominators are <= 2048, so two different fractions differ
 *   by at least 2^-22 and equal fractions give equal floats: f32 order is exact rational order.
 * mvae_tanimoto_knn: for each of Q queries (q [Q, 16]) row i of sim / idx ([Q, k], dense) holds the k eligible rows of table [N, 16] with
 *   the largest similarity, ordered by (similarity descending, row ascending).  Every row is eligible except exclude[i] (exclude [Q] int64
 *   or NULL; -1 = none).  With fewer than k eligible rows the tail of the output row is (-1.0f, -1).  Every element of sim and idx is
 *   written, nothing else is.  A query's answer does not depend on Q, on the other queries or on how the launch is laid out; two runs are
 *   bitwise equal.  Nothing of size Q x N exists: one scan launch keeps a k-entry list per (query, wave) in LDS (as exact fractions; the
 *   division happens where a result is written), and, when the table rows are split over `slots` partial lists per query to fill the chip
 *   (slots depends on Q and N alone, <= 256), one merge launch combines them.  Workspace: mvae_tanimoto_knn_workspace(Q, N, k) = slots *
 *   Q * k * 12 bytes (8-byte aligned; 0: one slot, none needed); it depends on (Q, N, k) alone.
 *   Refused before anything is enqueued.  MVAE_ERR_INVALID: a NULL or misaligned pointer other than exclude; Q, N or k < 1.
 *   MVAE_ERR_UNSUPPORTED: k > 32 (the workspace function then returns 0).  MVAE_ERR_WORKSPACE: a missing or short workspace.
 * mvae_tanimoto_sum: out[0] (float64, device) = the sum of the f32 similarities over all M x N ordered pairs of a [M, 16] and b [N, 16];
 *   with skip_diagonal != 0 the pairs with i == j are left out.  Accumulated in float64 in a fixed order (per lane over a's rows, a fixed
 *   tree per block, then one block over the per-block partials): two runs are bitwise equal, and no floating-point atomic is used.
 *   Internal diversity: IntDiv = 1 - sum / (M * M) with a == b is the MOSES form, diagonal included; skip_diagonal and M * (M - 1) give
 *   the other convention.  Workspace: mvae_tanimoto_sum_workspace(M, N) bytes (8-byte aligned, never 0; it depends on (M, N) alone).
 *   Refused before anything is enqueued.  MVAE_ERR_INVALID: a NULL or misaligned a / b, a NULL out, M or N < 1.  MVAE_ERR_WORKSPACE: a
 *   missing or short workspace.
 */
size_t mvae_tanimoto_knn_workspace(int Q, int64_t N, int k);
int mvae_tanimoto_knn(int Q, int64_t N, int k, const int64_t* q /* [Q, 16] */, const int64_t* table /* [N, 16] */,
                      const int64_t* exclude /* [Q] or NULL, -1 = none */, float* sim /* [Q, k] */, int64_t* idx /* [Q, k] */, void* ws,
                      size_t ws_bytes, void* stream);
size_t mvae_tanimoto_sum_workspace(int64_t M, int64_t N);
int mvae_tanimoto_sum(int64_t M, int64_t N, const int64_t* a /* [M, 16] */, const int64_t* b /* [N, 16] */, int skip_diagonal,
                      double* out /* [1] */, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Optimiser surface (K14 + K15): torch.nn.utils.clip_grad_norm_(params, max_norm) (train.py:102) followed by
 * torch.optim.Adam.step() (train.py:81,104) on a FLAT fp32 parameter / gradient / m / v buffer.
 *   mvae_sumsq: partial[i] = sum of squares of chunk i (deterministic); norm_out[0] = sqrt(total) is
 *   produced on device by mvae_clip_adam itself from `partial` (no host synchronisation).
 *   coef = min(1, max_norm / (norm + 1e-6)) (max_norm <= 0: no clipping); grads are scaled by
 *   grad_scale first (1/world_size after an all-reduce SUM).
 *   A step whose global norm is NOT FINITE is skipped as a whole: p, m, v stay as they are and norm_out[1] (when norm_out has room for it:
 *   norm_out_len >= 2) is incremented by one.  That is how a failed persistent launch (mvae_rnn_*_desc.poison -> a NaN in a slot of g that
 *   mvae_sumsq covers) keeps the weights intact without any host synchronisation; the reference would turn every parameter into NaN at
 *   such a step (clip_grad_norm_ scales by NaN).  poison_reset (optional): that slot, set back to 0 by the launch for the next step.
 */
size_t mvae_sumsq_workspace(int64_t n);
int mvae_sumsq(int64_t n, const float* g, float* partial, void* stream);
int mvae_clip_adam(int64_t n, float* p, const float* g, float* m, float* v, const float* partial, int64_t npartial,
                   float grad_scale, float max_norm, float lr, float beta1, float beta2, float eps, int step,
                   float* norm_out, int norm_out_len, float* poison_reset, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * The same clip followed by torch.optim.SGD.step() (train_distributed.py:73,91) on a FLAT fp32 parameter / gradient /
 * momentum buffer.  Reads the partial sums of mvae_sumsq exactly as mvae_clip_adam does (same norm, same coef, same
 * skip of a step whose norm is not finite, same norm_out / poison_reset), then per element, in torch's order:
 *   d = g * coef + weight_decay * p
 *   momentum != 0: buf = initialised ? momentum * buf + (1 - dampening) * d : d;   d = nesterov ? d + momentum * buf : buf
 *   p -= lr * d
 * momentum == 0: buf and initialised are not touched (may be NULL): 12 bytes per element instead of 20.
 * initialised [2] (momentum != 0): torch's "momentum_buffer is not None", as a device word double-buffered by the host's step
 * parity: the launch reads initialised[parity] and writes initialised[parity ^ 1] (1 after an update; a skipped step copies the
 * word it read), so no block of a launch reads what another block of the same launch writes.  The caller alternates parity
 * step by step, and sets both words when it loads a state.
 * Rejected (MVAE_ERR_INVALID, before anything is enqueued): n < 0, npartial < 1, momentum < 0, nesterov with momentum <= 0 or
 * dampening != 0, parity not 0 / 1, a NULL buffer that the arguments need.
 */
int mvae_clip_sgd(int64_t n, float* p, const float* g, float* buf, const float* partial, int64_t npartial, float grad_scale,
                  float max_norm, float lr, float momentum, float dampening, float weight_decay, int nesterov, int32_t* initialised,
                  int parity, float* norm_out, int norm_out_len, float* poison_reset, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MVAE_H_ */
