// Internal launcher declarations (host side).  The extern "C" surface is include/mvae.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include "../../include/mvae.h"
#include "launch.hpp"

size_t gemm_nt_workspace_bytes(int M, int N, int K, int dtype);
int launch_gemm_nt(int dtype, int M, int N, int K, const void* A, long lda, const void* B, long ldb, void* C, long ldc,
                   int c_dtype, const float* bias, int act, int accumulate, void* ws, size_t ws_bytes, hipStream_t st);
int launch_gemm_nt_grouped(int dtype, int M, int N, int K, const void* A, long lda, int a_group, long a_gstride, long a_total,
                           const void* B, long ldb, void* C, long ldc, int c_dtype, const float* bias, int act, int accumulate,
                           void* ws, size_t ws_bytes, hipStream_t st);
size_t gemm_tn_f32_workspace_bytes(int M, int N, int R);
int launch_gemm_tn_f32(int M, int N, int R, const float* A, long lda, int a_group, long a_gstride, const float* B, long ldb, int b_group,
                       long b_gstride, float* C, long ldc, int accumulate, void* ws, size_t ws_bytes, hipStream_t st, bool x3 = false,
                       float* colsum_out = nullptr, int colsum_acc = 0);
size_t gemm_tn_workspace_bytes(int M, int N, int K);
int launch_gemm_tn_bf16(int M, int N, int K, const void* A, long lda, const void* B, long ldb, void* C, long ldc, int c_dtype,
                        const float* bias, int act, int accumulate, void* ws, size_t ws_bytes, hipStream_t st);
bool gemm_tn_colsum_supported(int M, int N, int K);
size_t gemm_tn_colsum_workspace_bytes(int M, int N, int K);
int launch_gemm_tn_bf16_colsum(int M, int N, int K, const void* A, long lda, const void* B, long ldb, void* C, long ldc, int c_dtype,
                               const float* bias, int act, int accumulate, float* colsum_out, int colsum_acc, void* ws, size_t ws_bytes,
                               hipStream_t st);
int launch_cast_transpose(int dsrc, int ddst, int R, int C, const void* src, long lds_, void* dst, long ldd, void* dstT,
                          long ldt, hipStream_t st);
size_t colsum_workspace_bytes(int M, int N);
int launch_colsum(int M, int N, const float* X, long ldx, float* out, void* ws, size_t ws_bytes, hipStream_t st);
int launch_selu_bwd(long n, float* dy, const float* y, hipStream_t st);
// corpus_index.hip: the exact hash index over the CSR corpus (both check their arguments before anything is enqueued)
int launch_corpus_index_build(const uint8_t* tokens, const int64_t* offsets, int64_t N, int64_t* slots, int64_t n_slots, int64_t* n_distinct,
                              hipStream_t st);
int launch_corpus_index_probe(const uint8_t* tokens, const int64_t* offsets, int64_t N, const int64_t* slots, int64_t n_slots, int B, int T,
                              const int64_t* x, int64_t x_ld, int eos, int64_t* match, hipStream_t st);

// Where the launches of the current mvae_rnn_fwd / mvae_rnn_bwd call report a bounded spin that ran out (capi.hip clears it before dispatching
// and hands it to the caller as *status_out): set by every launcher that enqueues a kernel with bounded spins, left alone by the others.
extern thread_local const void* mvae_tls_status;

// rnn_persist.hip: weights-resident dataflow LSTM forward (b = 128, 4 x 1024, bf16)
bool rnn_persist_fwd_supported(const mvae_rnn_fwd_desc* d);
size_t rnn_persist_fwd_workspace_bytes(int T);
int rnn_persist_fwd(const mvae_rnn_fwd_desc* d, void* ws, size_t ws_bytes, hipStream_t st);
// rnn_persist_bwd.hip: weights-resident dataflow LSTM backward (same shape)
bool rnn_persist_bwd_supported(const mvae_rnn_bwd_desc* d);
size_t rnn_persist_bwd_workspace_bytes(int T);
int rnn_persist_bwd(const mvae_rnn_bwd_desc* d, void* ws, size_t ws_bytes, hipStream_t st);
// rnn_rowres.hip: row-resident schedules (narrow f32 LSTM stacks; the one-layer bf16 GRU(256)); MVAE_ERR_UNSUPPORTED = not their shape
size_t rnn_rowres_fwd_pipe_workspace(const mvae_rnn_fwd_desc* d);     // layer-concurrent LSTM forward: 0 = shape / device not served
int rnn_rowres_fwd(const mvae_rnn_fwd_desc* d, hipStream_t st);
size_t rnn_rowres_bwd_workspace(int layers, int T, int B, int H);
int rnn_rowres_bwd(const mvae_rnn_bwd_desc* d, hipStream_t st);
int rnn_gru_rowres_fwd(const mvae_rnn_fwd_desc* d, hipStream_t st);
int rnn_gru_rowres_bwd(const mvae_rnn_bwd_desc* d, hipStream_t st);
// rnn.hip: argument checks, then the row-resident schedules where they serve the shape, else the layer-wavefront launches
int rnn_fwd_impl(const mvae_rnn_fwd_desc* d, hipStream_t st);
int rnn_bwd_impl(const mvae_rnn_bwd_desc* d, hipStream_t st);
size_t rnn_bwd_workspace_bytes(const mvae_rnn_bwd_desc* d);
