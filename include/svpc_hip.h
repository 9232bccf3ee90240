/* svpc_hip.h — C-ABI of the MI355X (gfx950) kernel library behind svpc_amd's StateAwareRecursiveTransformer.
 *
 * The reference (awkrail/svpc) has no FFI / plugin layer: its hot path is eager PyTorch inside
 * src/rtransformer/model.py.  The drop-in boundary is therefore the Python module API; this
 * header is what sits directly beneath it.  Each entry point replaces the group of eager ops cited next to it
 * (paths relative to the reference root).  INTEGRATION.md shows the ctypes binding a maintainer adds.
 *
 * Conventions: every pointer is a device (HBM) pointer unless noted; tensors are row-major fp32 / int32;
 * `stream` is the HIP stream to launch on (svpc_amd passes PyTorch's current stream); nothing is allocated
 * and nothing synchronises inside (graph-capture safe); return 0 = ok, non-zero = error with a message in
 * svpc_last_error().  Dropout / Gumbel draws are counter-based: (`seed` device word, `site`, element index).
 */
#ifndef SVPC_HIP_H
#define SVPC_HIP_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* svpc_stream_t; /* == hipStream_t */
typedef unsigned long long svpc_u64;

#define SVPC_ACT_NONE 0
#define SVPC_ACT_RELU 1
#define SVPC_ACT_GELU 2    /* exact erf GELU, model.py:58-64 */
#define SVPC_ACT_SIGMOID 3

const char* svpc_last_error(void);
int svpc_abi_version(void);

/* ---- LayerNorm family: BertLayerNorm model.py:143-156 and its fused uses :229-233, :285-289, :493-499, :548-562,
 *      :650, :659, :889-891.  y = post_drop(LN(pre_drop(x[src_rows[r]]) + res[r])·gamma+beta) + add1[r%mod1] + add2[idx2[r]] */
int svpc_ln_fwd(const float* x, const int* src_rows, const float* res, const float* gamma, const float* beta, float* y,
                float* mean, float* rstd, int R, int D, float eps, float p_pre, unsigned site_pre, float p_post,
                unsigned site_post, const svpc_u64* seed, const float* add1, int mod1, const float* add2, const int* idx2,
                svpc_stream_t stream);
/* typed forms (dtype codes 0 = fp32, 1 = bf16; x_dt: x/dx, y_dt: residual/y/dy/dh; (0,0), (0,1), (1,1)); statistics stay fp32 */
int svpc_ln_fwd_t(const void* x, int x_dt, const int* src_rows, const void* res, const float* gamma, const float* beta, void* y,
                  int y_dt, float* mean, float* rstd, int R, int D, float eps, float p_pre, unsigned site_pre, float p_post,
                  unsigned site_post, const svpc_u64* seed, const float* add1, int mod1, const float* add2, const int* idx2,
                  svpc_stream_t stream);
int svpc_ln_bwd_t(const void* dy, const void* x, int x_dt, int y_dt, const int* src_rows, const void* res, const float* gamma,
                  const float* mean, const float* rstd, void* dh, void* dx, float* dgamma, float* dbeta, int accumulate,
                  float* workspace, int R, int D, float p_pre, unsigned site_pre, float p_post, unsigned site_post,
                  const svpc_u64* seed, svpc_stream_t stream);
/* the same in two calls, so that the parameter-gradient tail can run on another stream: partial = svpc_ln_bwd_groups(R)·2D floats */
int svpc_ln_bwd_rows_t(const void* dy, const void* x, int x_dt, int y_dt, const int* src_rows, const void* res, const float* gamma,
                       const float* mean, const float* rstd, void* dh, void* dx, float* partial, int R, int D, float p_pre,
                       unsigned site_pre, float p_post, unsigned site_post, const svpc_u64* seed, svpc_stream_t stream);
int svpc_ln_param_grads(const float* partial, int R, int D, float* dgamma, float* dbeta, int accumulate, svpc_stream_t stream);
/* strided / split forms (bf16x3 mode).  dtype code 2 = "split": a row stores an fp32-like value as TWO bf16 planes, hi = bf16(v) at
 * column c and lo = bf16(v - hi) at column lo + c (hi + lo is exact in fp32, 16-17 significant bits; the bytes of fp32).  ldx / ldr /
 * ldy: row strides in elements (0 = dense); lox / lor / loy: column offsets of the lo planes.  Forward combinations (x_dt, y_dt):
 * the typed ones plus (0,2), (2,2), (2,0).  The backward reads the hi planes of split rows in place as dtype 1 with their leading
 * dimension (ldx, ldr); dy / dh / dx stay dense.  Same reference lines as svpc_ln_fwd_t. */
int svpc_ln_fwd_s(const void* x, int x_dt, int ldx, int lox, const int* src_rows, const void* res, int ldr, int lor, const float* gamma,
                  const float* beta, void* y, int y_dt, int ldy, int loy, float* mean, float* rstd, int R, int D, float eps, float p_pre,
                  unsigned site_pre, float p_post, unsigned site_post, const svpc_u64* seed, const float* add1, int mod1,
                  const float* add2, const int* idx2, svpc_stream_t stream);
int svpc_ln_bwd_rows_s(const void* dy, const void* x, int x_dt, int ldx, int y_dt, const int* src_rows, const void* res, int ldr,
                       const float* gamma, const float* mean, const float* rstd, void* dh, void* dx, float* partial, int R, int D,
                       float p_pre, unsigned site_pre, float p_post, unsigned site_post, const svpc_u64* seed, svpc_stream_t stream);
int svpc_bucket_colsum_t(const void* x, int x_dt, int ldx, const int* idx, int R, int C, int K, float* out, int accumulate,
                         float* workspace, svpc_stream_t stream);
/* deferred reduction tails: the first stage of a plain column sum into a caller-owned partial buffer, and ONE launch that adds the
 * column sums of up to svpc_multi_finalize_max() partial buffers (bias gradients; LayerNorm [dgamma ; dbeta] with split = D) into
 * their arena targets: out(c) += Σ_g partial[g][c], c < split → out0[c], else out1[c - split].  `entries` is a HOST array. */
typedef struct svpc_finalize_entry { const float* partial; float* out0; float* out1; int groups, ncols, split; } svpc_finalize_entry;
int svpc_colsum_partial_t(const void* x, int x_dt, int ldx, int R, int C, float* partial, svpc_stream_t stream);
/* first stages of up to 48 plain column sums (dt: 0 = fp32, 1 = bf16 input) in one launch; partial_i = svpc_colsum_chunks(R_i) × C_i */
typedef struct svpc_colsum_entry { const void* x; float* partial; int dt, ldx, R, C; } svpc_colsum_entry;
int svpc_multi_colsum(const svpc_colsum_entry* entries, int n, svpc_stream_t stream);
int svpc_multi_finalize_max(void);
int svpc_multi_finalize(const svpc_finalize_entry* entries, int n, svpc_stream_t stream);
int svpc_ln_bwd_groups(int R); /* workspace floats needed by svpc_ln_bwd = (groups + 1) * 2 * D */
/* rows of `partial` that svpc_ln_bwd_rows_s writes when dh == dx == NULL (parameter gradients only: the first LayerNorm over the frame
 * features, model.py:548) — fewer, longer workgroups than the rows pass; svpc_ln_param_grads_g sums a given number of partial rows */
int svpc_ln_param_only_groups(int R);
int svpc_ln_param_grads_g(const float* partial, int groups, int D, float* dgamma, float* dbeta, int accumulate, svpc_stream_t stream);
int svpc_ln_bwd(const float* dy, const float* x, const int* src_rows, const float* res, const float* gamma,
                const float* mean, const float* rstd, float* dh, float* dx, float* dgamma, float* dbeta, int accumulate,
                float* workspace, int R, int D, float p_pre, unsigned site_pre, float p_post, unsigned site_post,
                const svpc_u64* seed, svpc_stream_t stream);
/* out[k][c] (+)= Σ_{r: idx[r]==k} x[r][c]  — bias gradients (K=1, idx NULL) and the token-type table gradient (model.py:890) */
int svpc_colsum_chunks(int R); /* workspace floats = chunks * K * C */
int svpc_bucket_colsum(const float* x, int ldx, const int* idx, int R, int C, int K, float* out, int accumulate,
                       float* workspace, svpc_stream_t stream);

/* ---- fp32 MFMA GEMM with fused epilogue: every nn.Linear on the path (model.py:195-197, :230, :259, :281, :496, :551,
 *      :706, :738, :755-770, :846-850, :859-860, nn.LSTM projections :865) and their dgrad / wgrad products.
 *      C[M,N] = epi(Σ_k A(m,k)·B(n,k)); a_kc/b_kc: 1 = k contiguous ([rows][ld]), 0 = k strided ([K][ld]). */
int svpc_gemm_f32(const float* A, int lda, int a_kc, const float* B, int ldb, int b_kc, float* C, int ldc, float* Z, int M, int N,
                  int K, const float* bias, int act, float p_drop, unsigned site, const svpc_u64* seed, int accumulate,
                  float* workspace, size_t workspace_bytes, svpc_stream_t stream);
/* same contract on the bf16 matrix cores (v_mfma_f32_32x32x16_bf16): fp32 operands are rounded to bf16 while staged, fp32 accumulate */
int svpc_gemm_bf16(const float* A, int lda, int a_kc, const float* B, int ldb, int b_kc, float* C, int ldc, float* Z, int M, int N,
                   int K, const float* bias, int act, float p_drop, unsigned site, const svpc_u64* seed, int accumulate,
                   float* workspace, size_t workspace_bytes, svpc_stream_t stream);
/* typed form (dtype codes 0 = fp32, 1 = bf16): (f32,f32→f32) any shape; (bf16,f32→bf16) NT/NN and (bf16,bf16→f32) TN for
 * interior-only shapes — the bf16 activation stream of the clip encoder */
int svpc_gemm_mx(const void* A, int a_dt, int lda, int a_kc, const void* B, int b_dt, int ldb, int b_kc, void* C, int c_dt, int ldc,
                 void* Z, int M, int N, int K, const float* bias, int act, float p_drop, unsigned site, const svpc_u64* seed,
                 int accumulate, float* workspace, size_t workspace_bytes, svpc_stream_t stream);
/* bf16 × bf16 form with direct-to-LDS operand staging (global_load_lds into an LDS ring, counted vmcnt): any M, N (see
 * svpc_gemm_glds_supported); weights come from the optimizer's bf16 shadow arena.  C bf16 (c_dt 1) or fp32 (c_dt 0).  Launches of
 * at least 200 tiles of 256x256 with a k-contiguous operand run on the two-group ping-pong kernel; bf16 outputs are written as whole
 * 128-byte lines. */
int svpc_gemm_glds_supported(int a_kc, int b_kc, int lda, int ldb, int M, int N, int K);
int svpc_gemm_glds(const void* A, int lda, int a_kc, const void* B, int ldb, int b_kc, void* C, int c_dt, int ldc, void* Z, int M, int N,
                   int K, const float* bias, int act, float p_drop, unsigned site, const svpc_u64* seed, int accumulate,
                   float* workspace, size_t workspace_bytes, svpc_stream_t stream);
/* the same with an addend R of C's type and leading dimension: C = epi(A·B) + R.  Lets the dgrad of a sub-layer's first projection
 * absorb the residual-path gradient (reference: the `+` of model.py:229-233 / :285-289 in backward) instead of a separate add kernel */
int svpc_gemm_glds_r(const void* A, int lda, int a_kc, const void* B, int ldb, int b_kc, void* C, int c_dt, int ldc, void* Z, const void* R,
                     int M, int N, int K, const float* bias, int act, float p_drop, unsigned site, const svpc_u64* seed, int accumulate,
                     float* workspace, size_t workspace_bytes, svpc_stream_t stream);
/* … and with an activation-backward factor G (of C's type and leading dimension): C = epi(A·B) ⊙ gact'(G) + R, where G is what the
 * forward of activation `gact` kept (the pre-activation z for GELU, the output y for ReLU / sigmoid).  The dgrad of the projection
 * that FOLLOWS an activation (reference: BertOutput.dense after BertIntermediate's gelu, model.py:255-289) writes the gradient of the
 * pre-activation directly; the separate svpc_act_bwd pass over the stream disappears.  G needs a non-accumulating bf16 output. */
int svpc_gemm_glds_rg(const void* A, int lda, int a_kc, const void* B, int ldb, int b_kc, void* C, int c_dt, int ldc, void* Z, const void* R,
                      const void* G, int gact, int M, int N, int K, const float* bias, int act, float p_drop, unsigned site,
                      const svpc_u64* seed, int accumulate, float* workspace, size_t workspace_bytes, svpc_stream_t stream);
/* the 8-phase 256x256x64 form of the same product for the FORWARD projections of a bf16 activation stream (both operands
 * k-contiguous bf16, bf16 output, optional bias / ReLU / GELU / pre-activation copy Z; K % 64 == 0, N % 8 == 0, 16-byte aligned rows):
 * C = act(A[M,K]·B[N,K]^T + bias).  svpc_gemm_glds routes its stream-sized forward launches here; the direct entry exists for tests
 * and tools.  reference: every nn.Linear of the clip encoder / decoder forward (model.py:195-197,230,259,281,551). */
int svpc_gemm_p8(const void* A, int lda, const void* B, int ldb, void* C, int ldc, void* Z, int M, int N, int K, const float* bias, int act,
                 svpc_stream_t stream);
/* bf16x3 form of the same projections (the ≤1e-4-parity throughput mode): split operands (see svpc_ln_fwd_s), three-term product
 *   A·Bᵀ ≈ A_lo·B_hiᵀ + A_hi·B_loᵀ + A_hi·B_hiᵀ   — one bf16 GEMM with a 3K-deep contraction on the svpc_gemm_p8 structure, fp32
 * accumulate, ≈2⁻¹⁷ per operand instead of 2⁻⁹ at 3× (not 16×, as the f32 MFMA) the bf16 matrix work.  A [M][lda]: hi plane at column
 * 0, lo plane at column a_lo; B_hi [N][ldb] with B_lo = B_hi + b_lo elements (same layout: the two planes of the weight shadow);
 * C [M][ldc] written split (hi at column c, lo at c_lo + c); Z (optional, only with an activation): plain bf16 [M][ldz] pre-activation
 * copy for the bf16 backward.  K % 64 == 0, N % 8 == 0, every plane 16-byte aligned; act in {none, relu, gelu}. */
int svpc_gemm_p8x3_supported(int lda, int a_lo, int ldb, int ldc, int c_lo, int ldz, int M, int N, int K);
int svpc_gemm_p8x3(const void* A, int lda, int a_lo, const void* B, int ldb, long long b_lo, void* C, int ldc, int c_lo, void* Z, int ldz,
                   int M, int N, int K, const float* bias, int act, svpc_stream_t stream);
/* the same contract on 128x128 tiles (4 waves, two workgroups per CU): the decoder's projections (4,224 sentence rows, 576 memory
 * rows; model.py:620-663), where 256x256 tiles leave most of the 256 CUs idle */
int svpc_gemm_s4x3(const void* A, int lda, int a_lo, const void* B, int ldb, long long b_lo, void* C, int ldc, int c_lo, void* Z, int ldz,
                   int M, int N, int K, const float* bias, int act, svpc_stream_t stream);
/* bf16 GEMM with a k-STRIDED B operand on the same 8-phase template — the input gradients (dgrad) of the stream projections:
 *   C[M,N] = (A[M,K] · B[K,N]) ⊙ gact'(G[M,N]) + R[M,N],  A = dz (k-contiguous), B = the weight matrix as stored (W[out = K][in = N]),
 * G (optional) what the forward of the activation in front of this projection's input kept, R (optional) a parked residual-path gradient;
 * all bf16, C / G / R share ldc.  K % 64 == 0, N % 8 == 0.  B fragments come from a [64 k-rows][128 columns] LDS image through
 * ds_read_b64_tr_b16.  reference: the backward of every nn.Linear of the clip encoder (model.py:195-197,230,259,281,551). */
/* the same dgrad on 128x128 tiles, 8 waves, up to four 32-KiB stages: the decoder's projections with M = 4,224 or 576 rows, where a
   256x256 tiling leaves most CUs idle. gemm_s4t.hip; replaces the backward of the nn.Linear layers of BertDecoderLayerNoMemoryUntied,
   src/rtransformer/model.py:620-663.  C = A·B + R with R optional; no activation factor. */
int svpc_gemm_s4t_supported(int lda, int ldb, int ldc, int M, int N, int K);
int svpc_gemm_s4t(const void* A, int lda, const void* B, int ldb, void* C, int ldc, const void* R, int M, int N, int K, svpc_stream_t stream);
int svpc_gemm_p8t_supported(int lda, int ldb, int ldc, int M, int N, int K);
int svpc_gemm_p8t(const void* A, int lda, const void* B, int ldb, void* C, int ldc, const void* G, int gact, const void* R, int M, int N, int K,
                  svpc_stream_t stream);
/* fp32-operand form with direct-to-LDS staging (deep LDS ring, operands rounded to bf16 when the MFMA fragments are built): the
 * latency-bound GEMMs of the decoder :620-694, step-wise encoder :594-617, simulators :742-823, BiLSTM :1017-1025, LM head
 * :697-739 and their dgrad/wgrad.  Any M, N (edges clamped); K % 32 == 0; k-strided operands need rows % 4 == 0. */
int svpc_gemm_l32_supported(int a_kc, int b_kc, int lda, int ldb, int M, int N, int K);
int svpc_gemm_l32_preferred(int a_kc, int b_kc, int lda, int ldb, int M, int N, int K);   /* supported AND measured faster */
int svpc_gemm_l32(const float* A, int lda, int a_kc, const float* B, int ldb, int b_kc, float* C, int ldc, float* Z, int M, int N, int K,
                  const float* bias, int act, float p_drop, unsigned site, const svpc_u64* seed, int accumulate, float* workspace,
                  size_t workspace_bytes, svpc_stream_t stream);
/* the same with an fp32 addend R of C's leading dimension, C = epi(A·B) + R (fp32 twin of svpc_gemm_glds_r: the residual-path
 * gradient of a LayerNorm joins the dgrad of the projection that consumes the residual tensor — step-wise encoder, model.py:565-591) */
int svpc_gemm_l32_r(const float* A, int lda, int a_kc, const float* B, int ldb, int b_kc, float* C, int ldc, float* Z, const float* R, int M,
                    int N, int K, const float* bias, int act, float p_drop, unsigned site, const svpc_u64* seed, int accumulate,
                    float* workspace, size_t workspace_bytes, svpc_stream_t stream);
/* ... and with the activation-backward factor, C = (A·B) * gact'(G) + R: G in fp32 and C's layout is what the forward of activation gact
 * kept, z for GELU, y for ReLU or sigmoid. The dgrad of the projection that consumes an activated tensor writes the gradient of the
 * pre-activation directly: the FFN of the step-wise encoder, model.py:565-591. No bias, activation or dropout in this form. */
int svpc_gemm_l32_rg(const float* A, int lda, int a_kc, const float* B, int ldb, int b_kc, float* C, int ldc, const float* R, const float* G,
                     int gact, int M, int N, int K, int accumulate, float* workspace, size_t workspace_bytes, svpc_stream_t stream);
/* the same contract with bf16x3 products: every fp32 operand value enters as hi + lo bf16 terms when the MFMA fragments are built,
 * three MFMAs per product — the forward arithmetic of the ≤1e-4-parity throughput mode for every projection in fp32 storage */
int svpc_gemm_l32_x3(const float* A, int lda, int a_kc, const float* B, int ldb, int b_kc, float* C, int ldc, float* Z, const float* R, int M,
                     int N, int K, const float* bias, int act, float p_drop, unsigned site, const svpc_u64* seed, int accumulate,
                     float* workspace, size_t workspace_bytes, svpc_stream_t stream);
/* grouped weight (+ bias) gradients of up to svpc_gemm_group_wgrad_max() independent linears in one launch:
 *   dw[n_out, n_in] += dzᵀ · x,   db[n_out] += Σ_rows dz   (db may be NULL)       — the wgrad half of every nn.Linear backward
 * `problems` is a HOST array of svpc_wgrad_problem; any row count (the partial last k-tile is zero-sourced), n_out % 4 == 0, n_in % 4 == 0,
 * 16-byte aligned operands */
/* grouped small GEMMs of one layout in one launch (fp32 operands, bf16 MFMA): C_p = (accumulate ? C_p : 0) + Σ_k A_p(m,k)·B_p(n,k);
 * `problems` is a HOST array, at most 32 entries, K % 32 == 0 — e.g. the recurrent projections of both LSTM directions at one step */
typedef struct svpc_gemm_problem { const float* A; const float* B; float* C; int M, N, K, lda, ldb, ldc; } svpc_gemm_problem;
int svpc_gemm_group(const svpc_gemm_problem* problems, int n, int a_kc, int b_kc, int accumulate, svpc_stream_t stream);
int svpc_gemm_group_x3(const svpc_gemm_problem* problems, int n, int a_kc, int b_kc, int accumulate, svpc_stream_t stream); /* bf16x3 products */
typedef struct svpc_wgrad_problem {
    const float* dz; const float* x; float* dw; float* db;
    int n_out, n_in, rows, ld_dz, ld_x, ld_dw;
} svpc_wgrad_problem;
int svpc_gemm_group_wgrad_max(void);
/* the bf16-stream table (svpc_gemm_group_wgrad_bf16_ws below) on the 8-phase 256x256x64 template with BOTH operands read k-strided through
 * ds_read_b64_tr_b16 (gemm_p8w.hip): problems at least 256 wide both ways; same balance (deep tiles of later rounds cut into k-parts →
 * fp32 slabs in `workspace`, added in part order by a fix-up launch).  _ok: 1 if every problem of the table qualifies. */
int svpc_gemm_group_wgrad_bf16_p8_ok(const void* problems, int n);
int svpc_gemm_group_wgrad_bf16_p8(const void* problems, int n, float* workspace, size_t workspace_bytes, svpc_stream_t stream);
/* the same for the bf16 activation streams (dz, x bf16; dw fp32; db must be NULL; n_out % 8 == 0, n_in % 8 == 0, any row count):
 * every 128² tile runs its whole k-loop — no split-K slabs, no reduce launches */
int svpc_gemm_group_wgrad_bf16(const svpc_wgrad_problem* problems, int n, svpc_stream_t stream);
/* the same with scratch for load balancing: deep tiles dealt after the first round of workgroups are cut into k-parts that write
 * fp32 slabs into `workspace`; a second launch adds a tile's slabs in part order into dW (deterministic) */
int svpc_gemm_group_wgrad_bf16_ws(const svpc_wgrad_problem* problems, int n, float* workspace, size_t workspace_bytes,
                                  svpc_stream_t stream);
int svpc_gemm_group_wgrad(const svpc_wgrad_problem* problems, int n, svpc_stream_t stream);
/* dz = dy · act'(aux) · dropout  (aux = pre-activation for GELU, activated output for ReLU / sigmoid) */
int svpc_act_bwd(const float* dy, const float* aux, float* dz, size_t n, int act, float p, unsigned site, const svpc_u64* seed,
                 svpc_stream_t stream);

int svpc_act_bwd_t(const void* dy, const void* aux, void* dz, int dt, size_t n, int act, float p, unsigned site, const svpc_u64* seed,
                   svpc_stream_t stream);

/* ---- attention core: BertSelfAttention.forward model.py:194-219 (scale, additive -10000 mask, softmax, dropout, PV).
 *      seq = int32[4][n_seq]: q_off, q_len, k_off, k_len.  LSE: (n_seq, H, max_q). */
int svpc_attn_fwd(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, float* O, int ldo, float* LSE,
                  const int* seq, int n_seq, int H, int dh, int max_q, int max_k, const float* key_mask, int causal, float scale,
                  float p_drop, unsigned site, const svpc_u64* seed, svpc_stream_t stream);
/* single-query form for incremental greedy decoding (src/translator.py:88-100: position i attends to positions ≤ i): every sequence
 * has exactly one query row; fp32, forward only */
int svpc_attn_q1_fwd(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, float* O, int ldo, float* LSE,
                     const int* seq, int n_seq, int H, int dh, int max_k, const float* key_mask, float scale, svpc_stream_t stream);
/* one decoding step of an attention block of the decoder layer (src/rtransformer/model.py:620-663 evaluated for ONE new position per
 * sentence, as src/translator.py:88-112 needs): O[t] = LayerNorm(X[t] + Attention(Q[t]; rows t·k_stride … t·k_stride+n_keys−1 of K / V)),
 * heads of dh = 64, fp32.  newK / newV (both or neither): the token's own key / value row, stored as row t·k_stride+n_keys−1 of the cache
 * before it is attended to (incremental self-attention); without them K / V are only read (cross-attention over the memory rows). */
int svpc_attn_q1_ln_supported(int D, int dh, int n_keys, int ldq, int ldkv, int ldnew, int ldx, int ldo);
int svpc_attn_q1_ln_fwd(const float* Q, int ldq, float* K, float* V, int ldkv, int k_stride, int n_keys, const float* newK, const float* newV,
                        int ldnew, const float* X, int ldx, const float* gamma, const float* beta, float eps, float* O, int ldo, int T, int D,
                        int dh, float scale, svpc_stream_t stream);
/* the same block for beam search (src/translator.py:194-203, `--use_beam --beam_size`, src/test.py:207-209), over T = sentences × B
 * hypothesis rows: with key_rows ((T, ld_rows) int32, the ancestry table svpc_beam_step writes) query t attends to rows key_rows[t·ld_rows + j],
 * j < n_keys, of K / V, and newK / newV are first stored at key_rows[t·ld_rows + n_keys − 1] — each hypothesis reads its ancestors' rows
 * where they were written, the caches are never copied or reordered.  key_rows == NULL: query t reads rows (t / q_group)·k_stride + j
 * (the B hypotheses of a sentence share its memory rows in the cross-attention).  Same shape limits as svpc_attn_q1_ln_fwd. */
int svpc_attn_q1_ln_idx_fwd(const float* Q, int ldq, float* K, float* V, int ldkv, int k_stride, int n_keys, const int* key_rows, int ld_rows,
                            int q_group, const float* newK, const float* newV, int ldnew, const float* X, int ldx, const float* gamma,
                            const float* beta, float eps, float* O, int ldo, int T, int D, int dh, float scale, svpc_stream_t stream);
int svpc_attn_bwd(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, const float* O, int ldo,
                  const float* LSE, const float* dO, int lddo, float* dQ, int lddq, float* dK, int lddk, float* dV, int lddv,
                  float* delta, const int* seq, int n_seq, int H, int dh, int max_q, int max_k, const float* key_mask, int causal,
                  float scale, float p_drop, unsigned site, const svpc_u64* seed, svpc_stream_t stream);

/* MFMA (bf16 operands, fp32 softmax/accumulate) form of the same core for ≤128×128 (queries×keys) per sequence, dh 32/64 */
int svpc_attn_mfma_supported(int dh, int max_q, int max_k, int ldq, int ldk, int ldv, int dt /* 0 fp32, 1 bf16: the leading dimensions are
                             checked in 16-byte units of that element type */);
int svpc_attn_mfma_fwd(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, float* O, int ldo, float* LSE,
                       const int* seq, int n_seq, int H, int dh, int max_q, int max_k, const float* key_mask, int causal,
                       float scale, float p_drop, unsigned site, const svpc_u64* seed, svpc_stream_t stream);
int svpc_attn_mfma_bwd(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, const float* O, int ldo,
                       const float* LSE, const float* dO, int lddo, float* dQ, int lddq, float* dK, int lddk, float* dV, int lddv,
                       const int* seq, int n_seq, int H, int dh, int max_q, int max_k, const float* key_mask, int causal, float scale,
                       float p_drop, unsigned site, const svpc_u64* seed, svpc_stream_t stream);

int svpc_attn_mfma_fwd_t(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, void* O, int ldo, int dt, float* LSE,
                         const int* seq, int n_seq, int H, int dh, int max_q, int max_k, const float* key_mask, int causal,
                         float scale, float p_drop, unsigned site, const svpc_u64* seed, svpc_stream_t stream);
/* bf16x3 forward over split-stored Q / K / V / O (hi planes at the pointers with the rows' leading dimensions, lo planes q_lo / k_lo /
 * v_lo / o_lo elements behind them): Sᵀ and Oᵀ as three-term split-bf16 products, fp32 softmax, the library's dropout draws; non-causal,
 * ≤128 rows per sequence, head dim 32 / 64.  The backward is svpc_attn_mfma_bwd_t on the hi planes.  model.py:194-219 (clip encoder). */
int svpc_attn_stream_x3_fwd(const void* Q, int ldq, int q_lo, const void* K, int ldk, int k_lo, const void* V, int ldv, int v_lo, void* O,
                            int ldo, int o_lo, float* LSE, const int* seq, int n_seq, int H, int dh, int max_q, int max_k,
                            const float* key_mask, float scale, float p_drop, unsigned site, const svpc_u64* seed, svpc_stream_t stream);
/* one fp32 query per sequence against bf16 (k_lo = v_lo = 0) or split keys / values, forward and backward — the [CLS]-only last
 * clip-encoder layer of the training forward (model.py:1062-1064; core :194-219): a wave per (sequence, head), exact fp32 arithmetic on
 * the values read, no LDS; <= 128 keys, head dim 32 / 64.  Backward: dQ fp32, dK / dV dense bf16 rows (every key row is written). */
int svpc_attn_q1s_supported(int dh, int max_k, int ldq, int ldk, int ldv, int k_lo, int v_lo);
int svpc_attn_q1s_fwd(const float* Q, int ldq, const void* K, int ldk, int k_lo, const void* V, int ldv, int v_lo, float* O, int ldo, float* LSE,
                      const int* seq, int n_seq, int H, int dh, int max_k, const float* key_mask, float scale, float p_drop, unsigned site,
                      const svpc_u64* seed, svpc_stream_t stream);
int svpc_attn_q1s_bwd(const float* Q, int ldq, const void* K, int ldk, int k_lo, const void* V, int ldv, int v_lo, const float* dO, int lddo,
                      float* dQ, int lddq, void* dK, int lddk, void* dV, int lddv, const int* seq, int n_seq, int H, int dh, int max_k,
                      const float* key_mask, float scale, float p_drop, unsigned site, const svpc_u64* seed, svpc_stream_t stream);
/* general bf16x3 forward: sequences of <= 32 queries and keys (the decoder's causal self-attention and its memory cross-attention,
 * model.py:620-663) run one wave per (sequence, head) and may be causal; longer ones take the stream kernel above (non-causal) */
int svpc_attn_x3_fwd(const void* Q, int ldq, int q_lo, const void* K, int ldk, int k_lo, const void* V, int ldv, int v_lo, void* O, int ldo,
                     int o_lo, float* LSE, const int* seq, int n_seq, int H, int dh, int max_q, int max_k, const float* key_mask, int causal,
                     float scale, float p_drop, unsigned site, const svpc_u64* seed, svpc_stream_t stream);
/* Sequences of 33-104 rows (the clip encoder's 100 x 100 x 64) of the bf16 / split streams take a PERSISTENT forward inside
 * svpc_attn_mfma_fwd_t / svpc_attn_x3_fwd (attention_pipe.hip: a loader wave keeps the K / V planes of the next two (sequence, head)
 * pairs in flight by LDS-DMA while four waves compute the current one; same arithmetic, dropout draws and LSE).  This switch selects
 * it (1, default), the one-workgroup-per-pair kernels (0), or just reports (negative); returns the previous setting.  A/B use only. */
int svpc_attn_pipe_enable(int on);
/* timing experiments on that kernel (tools/dbg/pipe_phases.py, pipe_stamps.py): bits 1 no LDS-DMA, 2 no arithmetic, 4 no O stores,
 * 8 no Q loads, 16 s_memtime stamps of workgroups 0-15 into buf (16 x 128 u64 of device memory).  0 / NULL = production. */
int svpc_attn_pipe_debug(int bits, void* buf);
int svpc_attn_mfma_bwd_t(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, const void* O, int ldo, int dt,
                         const float* LSE, const void* dO, int lddo, void* dQ, int lddq, void* dK, int lddk, void* dV, int lddv,
                         const int* seq, int n_seq, int H, int dh, int max_q, int max_k, const float* key_mask, int causal, float scale,
                         float p_drop, unsigned site, const svpc_u64* seed, svpc_stream_t stream);

/* ---- simulator recurrence: EntitiyReasoningNetwork.forward model.py:792-820 (Eqs. 2-7), one workgroup per video */
int svpc_sim_recur_fwd(const float* q, const float* c, const float* w4f, const float* E0, const int* step_off, const int* step_len,
                       const int* ent_off, const int* ent_len, int n_videos, int e_max, int D, float* e_out, float* ebar,
                       float* eall, svpc_stream_t stream);
int svpc_sim_recur_bwd(const float* q, const float* c, const float* w4f, const float* E0, const int* step_off, const int* step_len,
                       const int* ent_off, const int* ent_len, int n_videos, int e_max, int D, const float* e_out,
                       const float* ebar, const float* eall, const float* de, const float* debar, const float* deall, float* dq,
                       float* dc, float* dw4f, float* dE0, svpc_stream_t stream);

/* the simulator's two tiny heads in one launch each way: c = softmax(hh·W3^T + b3) (three choice weights per step, src/rtransformer/model.py:801)
 * and w = fb·W4^T + b4 (one scalar per step, :804-805).  Backward: dhh (T, D) and dfb (T, Wd) fully written; the weight / bias gradients as
 * per-workgroup partial sums part3 (groups, 3·D + 3) = [dW3 | db3], part4 (groups, Wd + 1) = [dW4 | db4], groups = svpc_sim_heads_groups(T),
 * for svpc_multi_finalize.  dc / dw may be NULL (no gradient). */
int svpc_sim_heads_groups(int T);
int svpc_sim_heads_fwd(const float* hh, const float* fb, const float* W3, const float* b3, const float* W4, const float* b4, float* c, float* w,
                       int T, int D, int Wd, svpc_stream_t stream);
int svpc_sim_heads_bwd(const float* hh, const float* fb, const float* W3, const float* W4, const float* c, const float* dc, const float* dw,
                       float* dhh, float* dfb, float* part3, float* part4, int T, int D, int Wd, svpc_stream_t stream);

/* ---- decoder cross-attention over the <= 3 memory rows of a sentence + residual LayerNorm, one launch forward and one backward per
 * layer: src/rtransformer/model.py:657-658 (BertDecoderLayerNoMemoryUntied.forward), attention core :194-219, BertLayerNorm :143-156.
 *   y = LayerNorm(x1 + MHA(query rows q; keys / values = the sentence's nm memory rows))
 * q, x1: T·lt rows; k, v: T·nm rows (the layer's key / value column blocks of the memory projection).  dt codes: 0 fp32, 1 bf16, 2 split (two
 * bf16 planes, the lo plane lo* columns behind).  probs (T·lt, H, 4), mean / rstd (T·lt) are saved for the backward, which returns the
 * gradients of the query rows and of the residual rows (dense, dg_dt), of the key / value rows (dense, dkv_dt, row stride ld_dkv) and the
 * per-sentence partial sums of [dgamma | dbeta] (T, 2D) for svpc_multi_finalize. */
int svpc_cross_attn_ln_supported(int D, int H, int lt, int nm);
int svpc_cross_attn_ln_fwd(const void* q, int q_dt, int ldq, int loq, const void* x1, int x_dt, int ldx, int lox, const void* k, const void* v,
                           int kv_dt, int ld_kv, int lokv, const float* gamma, const float* beta, float eps, void* y, int y_dt, int ldy, int loy,
                           float* probs, float* mean, float* rstd, int T, int lt, int nm, int D, int H, float scale, float p_drop, unsigned site,
                           const svpc_u64* seed, svpc_stream_t stream);
int svpc_cross_attn_ln_bwd(const void* q, int q_dt, int ldq, int loq, const void* x1, int x_dt, int ldx, int lox, const void* k, const void* v,
                           int kv_dt, int ld_kv, int lokv, const float* gamma, const float* probs, const float* mean, const float* rstd,
                           const void* dy, int dy_dt, int lddy, void* dq, void* dres, int dg_dt, int lddg, void* dk, void* dv, int dkv_dt,
                           int ld_dkv, float* part_ln, int T, int lt, int nm, int D, int H, float scale, float p_drop, unsigned site,
                           const svpc_u64* seed, svpc_stream_t stream);
/* the same over RAGGED sentences — the decoder run over the valid tokens only (nothing a pad token computes reaches the loss: model.py:630-640
 * masks pad keys, the caption loss ignores pad labels): sentence s owns the rows [row_off[s], row_off[s] + row_len[s]) of q, x1, y, probs, mean,
 * rstd, dy, dq, dres; row_len[s] <= lt, the padded length (register bound of the kernels, stride of the dropout rows); NULL, NULL = uniform */
int svpc_cross_attn_ln_fwd_r(const void* q, int q_dt, int ldq, int loq, const void* x1, int x_dt, int ldx, int lox, const void* k, const void* v,
                             int kv_dt, int ld_kv, int lokv, const float* gamma, const float* beta, float eps, void* y, int y_dt, int ldy, int loy,
                             float* probs, float* mean, float* rstd, int T, int lt, int nm, int D, int H, float scale, float p_drop, unsigned site,
                             const svpc_u64* seed, const int* row_off, const int* row_len, svpc_stream_t stream);
int svpc_cross_attn_ln_bwd_r(const void* q, int q_dt, int ldq, int loq, const void* x1, int x_dt, int ldx, int lox, const void* k, const void* v,
                             int kv_dt, int ld_kv, int lokv, const float* gamma, const float* probs, const float* mean, const float* rstd,
                             const void* dy, int dy_dt, int lddy, void* dq, void* dres, int dg_dt, int lddg, void* dk, void* dv, int dkv_dt,
                             int ld_dkv, float* part_ln, int T, int lt, int nm, int D, int H, float scale, float p_drop, unsigned site,
                             const svpc_u64* seed, const int* row_off, const int* row_len, svpc_stream_t stream);

/* ---- pointer-generator + caption loss: model.py:896-923, :37-55 */
int svpc_ptr_attn_fwd(const float* dec, const float* proj, const float* bank, const int* step_ne, float* pi, float* att, int T,
                      int lt, int e_max, int D, svpc_stream_t stream);
/* … with the generation gate p_gen = sigmoid([dec ; att]·w + b) (src/rtransformer/model.py:905-908) of every row computed in the same launch
 * (w: 2·D floats, b: one; att may be null): what a decoding iteration needs of the pointer, lt = 1 */
int svpc_ptr_attn_pgen_fwd(const float* dec, const float* proj, const float* bank, const int* step_ne, float* pi, float* att,
                           const float* pgen_w, const float* pgen_b, float* pgen, int T, int lt, int e_max, int D, svpc_stream_t stream);
int svpc_ptr_attn_bwd(const float* dec, const float* proj, const float* bank, const int* step_ne, const float* pi, const float* dpi,
                      const float* datt, float* ddec, float* dproj, float* dbank, int T, int lt, int e_max, int D,
                      svpc_stream_t stream);
/* training form: pointer attention AND the generation gate of every row in one launch, forward and backward (model.py:899-908).  The
 * attended vector feeds only the gate, so it never reaches HBM; backward returns the per-step partial sums of [d pgen_w | d pgen_b] in
 * wpart (T rows of 2·D + 1 floats) for the table-driven finalizer (svpc_multi_finalize). */
int svpc_ptr_attn_gate_fwd(const float* dec, const float* proj, const float* bank, const int* step_ne, float* pi, const float* pgen_w,
                           const float* pgen_b, float* pgen, int T, int lt, int e_max, int D, svpc_stream_t stream);
int svpc_ptr_attn_gate_bwd(const float* dec, const float* proj, const float* bank, const int* step_ne, const float* pi, const float* dpi,
                           const float* pgen, const float* dpgen, const float* pgen_w, float* ddec, float* dproj, float* dbank,
                           float* wpart, int T, int lt, int e_max, int D, svpc_stream_t stream);
/* the same two over RAGGED sentences — the head run over the valid tokens only (model.pack_text_rows): sentence j owns the rows
 * [row_off[j], row_off[j] + row_len[j]) of dec, pi, pgen (and of ddec, dpi, dpgen), row_len[j] <= lt (the padded length); NULL, NULL = uniform */
int svpc_ptr_attn_gate_fwd_r(const float* dec, const float* proj, const float* bank, const int* step_ne, float* pi, const float* pgen_w,
                             const float* pgen_b, float* pgen, int T, int lt, int e_max, int D, const int* row_off, const int* row_len,
                             svpc_stream_t stream);
int svpc_ptr_attn_gate_bwd_r(const float* dec, const float* proj, const float* bank, const int* step_ne, const float* pi, const float* dpi,
                             const float* pgen, const float* dpgen, const float* pgen_w, float* ddec, float* dproj, float* dbank,
                             float* wpart, int T, int lt, int e_max, int D, const int* row_off, const int* row_len, svpc_stream_t stream);
int svpc_ptr_mix_loss_fwd(const float* logits, const float* g, const float* pi, const int* labels, const int* row_c,
                          const int* row_vid, const int* csr_off, const int* csr_ent, const int* csr_id, const float* csr_w, float* P,
                          float* loss_rows, int R, int V, int c_max, int e_max, float smoothing, svpc_stream_t stream);
int svpc_ptr_mix_loss_bwd(const float* logits, const float* g, const float* pi, const int* labels, const int* row_c,
                          const int* row_vid, const int* csr_off, const int* csr_ent, const int* csr_id, const float* csr_w,
                          const float* P, const float* dP_ext, const float* dloss, float* dlogits, float* dg, float* dpi, int R, int V,
                          int c_max, int e_max, float smoothing, svpc_stream_t stream);
/* label_smoothing == 0: the reference then applies nn.CrossEntropyLoss(ignore_index=-1) to the PROBABILITIES (src/rtransformer/model.py:869-870
 * used at :960,982,1002,1014) — per video the mean over its non-ignored rows of logsumexp_{v<C}(P_v) − P_y.  row_w[r] = 1 / (valid rows of
 * row r's video), from svpc_ce_row_weights; loss_rows[r] = row_w[r]·(…) so that their sum is Σ_videos mean.  row_w == NULL: the
 * label-smoothed KL above (smoothing > 0 required). */
int svpc_ce_row_weights(const int* labels, const int* row_vid, int R, int n_vid, float* row_w, svpc_stream_t stream);
int svpc_ptr_mix_ce_fwd(const float* logits, const float* g, const float* pi, const int* labels, const int* row_c,
                        const int* row_vid, const int* csr_off, const int* csr_ent, const int* csr_id, const float* csr_w, float* P,
                        float* loss_rows, int R, int V, int c_max, int e_max, float smoothing, const float* row_w, svpc_stream_t stream);
int svpc_ptr_mix_ce_bwd(const float* logits, const float* g, const float* pi, const int* labels, const int* row_c,
                        const int* row_vid, const int* csr_off, const int* csr_ent, const int* csr_id, const float* csr_w,
                        const float* P, const float* dP_ext, const float* dloss, float* dlogits, float* dg, float* dpi, int R, int V,
                        int c_max, int e_max, float smoothing, const float* row_w, svpc_stream_t stream);

/* ---- Gumbel-softmax (hard) re-sampling of the caption: reconstruct model.py:1018 */
int svpc_gumbel_noise(float* out, size_t n, unsigned site, const svpc_u64* seed, svpc_stream_t stream);
int svpc_gumbel_fwd(const float* P, const float* noise, const int* row_c, const float* emb, float* bow, int* idx, float* stats, int R,
                    int c_max, int V, int W, float tau, svpc_stream_t stream);
int svpc_gumbel_bwd(const float* P, const float* noise, const int* row_c, const float* stats, const float* dy, float* dP, int R,
                    int c_max, int V, float tau, svpc_stream_t stream);
int svpc_gumbel_emb_grad(const float* dbow, const int* idx, const float* stats, float* demb, int R, int V, int W,
                         svpc_stream_t stream);

/* ---- row / span / loss kernels: Eq.(1) a/Σa model.py:798; softmax(W3 ĥ) :804; ingredient pooling :125-139; [CLS]+PE :1064;
 *      masked bag-of-words mean :1019-1021; nn.BCELoss(sum) :871; AsymmetricLoss libs/ASL/src/loss_functions/losses.py:15-50;
 *      nn.LSTM cell :865; nn.Embedding(padding_idx=0) gradient :492,:519 */
int svpc_rownorm_fwd(const float* a, float* y, int R, int C, int mode, svpc_stream_t stream);  /* mode 0: a/Σa, 1: softmax */
int svpc_rownorm_bwd(const float* dy, const float* y, const float* a, float* da, int R, int C, int mode, svpc_stream_t stream);
int svpc_span_mean_fwd(const float* x, const int* starts, const int* lens, const float* w, const float* add, const int* add_idx,
                       float* out, int G, int D, svpc_stream_t stream);
int svpc_span_mean_bwd(const float* dout, const int* starts, const int* lens, const float* w, float* dx, int G, int D,
                       svpc_stream_t stream);
int svpc_scatter_add_rows(const float* dx, const int* idx, float* dtable, int R, int D, int pad_row, svpc_stream_t stream);
int svpc_bce_rows_fwd(const float* p, const float* y, const int* widths, float* out, int R, int C, svpc_stream_t stream);
int svpc_bce_rows_bwd(const float* dout, const float* p, const float* y, const int* widths, float* dp, int R, int C,
                      svpc_stream_t stream);
int svpc_asl_rows_fwd(const float* p, const float* y, const float* active, float* out, int R, int C, float gneg, float gpos,
                      float clip, float eps, svpc_stream_t stream);
int svpc_asl_rows_bwd(const float* dout, const float* p, const float* y, const float* active, float* dp, int R, int C, float gneg,
                      float gpos, float clip, float eps, svpc_stream_t stream);
/* The whole loss sum in one launch (and its backward in one): total = sum(cap_rows) + [sum_r BCE(e_p[r], align[r]; first widths[r]
 * columns) + sum_{r: any(act[r] == 1)} ASL(a_p[r], act[r])] + lambda * [the same for the re-simulator's r_e / r_a] — reference
 * model.py:1110-1115 (per-video BCE-sum / ASL), :1168-1188 (re-simulation terms weighted by lambda_, total).  Any of e_p / a_p / r_e /
 * r_a may be NULL (modes without a simulator).  out5 = {total, caption, entity, action, re-simulation}.  Deterministic (row
 * partials in `workspace`, svpc_loss_tail_ws_floats() floats, summed in index order by the last workgroup; `counter`: one int zeroed
 * once by the caller, left at zero by every launch). */
int svpc_loss_tail_ws_floats(int n_cap, int R);
int svpc_loss_tail_fwd(const float* cap_rows, int n_cap, const float* e_p, const float* align, const int* widths, int R, int Ce,
                       const float* a_p, const float* act, int Ca, const float* r_e, const float* r_a, float lambda, float gneg,
                       float gpos, float clip, float eps, float* out5, float* workspace, int* counter, svpc_stream_t stream);
int svpc_loss_tail_bwd(const float* dout, int n_cap, const float* e_p, const float* align, const int* widths, int R, int Ce,
                       const float* a_p, const float* act, int Ca, const float* r_e, const float* r_a, float lambda, float gneg,
                       float gpos, float clip, float eps, float* d_cap, float* de_p, float* da_p, float* dr_e, float* dr_a,
                       svpc_stream_t stream);
int svpc_row_any_eq1(const float* x, float* out, int R, int C, svpc_stream_t stream);
/* token staging: up to 8 segments dst[i] = cast(src[idx ? idx[i] : i]) in one launch.  `segments`: array of
 *   struct { const void* src; const int* idx; void* dst; int src_dt, dst_dt, n; }   (dtype codes 0 fp32, 1 int64, 2 int32; dst fp32 / int32)
 * — the clip rows' and sentence rows' ids / masks / labels out of the loader's (step, video) tensors, reference train.py:91-112 +
 * model.py:1038-1042, 925-1015 (there: slicing inside a Python loop over steps and videos). */
int svpc_gather_cast_multi(const void* segments, int n, svpc_stream_t stream);
/* the same, advancing the step's dropout / Gumbel seed (the update of svpc_bump_seed) in the same launch when bump_seed != NULL */
int svpc_gather_cast_multi_seed(const void* segments, int n, svpc_u64* bump_seed, svpc_stream_t stream);
int svpc_clamp_labels(const int* in, int* out, int n, int vocab, int unk, svpc_stream_t stream); /* model.py:1013 */
int svpc_lstm_cell_fwd(const float* gx, const float* gh, const float* c_prev, const float* h_prev, const float* active, float* h,
                       float* c, float* gates_act, int N, int D, svpc_stream_t stream);
int svpc_lstm_cell_bwd(const float* dh, const float* dc, const float* gates_act, const float* c_prev, const float* active,
                       float* dgates, float* dc_prev, float* dh_prev, int N, int D, svpc_stream_t stream);
/* on-device logging counters (doubles in HBM; one read-back per logging interval instead of ≈10 .item() syncs per step):
 * src/train.py:32-38 cal_performance → counters[0] += #labelled rows, counters[1] += #rows whose first-index arg-max == label;
 * src/train.py:40-49 calculate_f1   → counters[0] += Σ gold[prob>0.5], [1] += Σ gold, [2] += #(prob>0.5) */
int svpc_metric_argmax(const float* scores, int ld, int R, int C, const long long* labels, int ignore, double* counters,
                       svpc_stream_t stream);
int svpc_metric_f1(const float* prob, const float* gold, size_t n, double* counters, svpc_stream_t stream);
/* input staging: gather the frame windows of a batch out of an HBM-resident feature bank (idx < 0 → zero row) —
 * recursive_caption_dataset.py:187-189 (resnet‖bn concat), :389-416 (window / down-sample / [CLS]…[SEP] layout), train.py:91 (H2D);
 * and the video half of input_ids / input_mask built on the device from the valid-frame counts (:409-415) */
int svpc_gather_rows_f32(const float* src, const int* idx, float* dst, int rows, int width, svpc_stream_t stream);
int svpc_video_tokens(const int* n_valid, long long* ids, float* mask, int clips, int Lv, int L, int cls_id, int vid_id, int sep_id,
                      int pad_id, svpc_stream_t stream);
/* sequence forms for the fused recurrence (nn.LSTM model.py:859-860, used at :1022-1024): gx rows gathered in place; the
 * backward adds the gradient from the layer above (dh_out) to the recurrent one (dh_rec) */
int svpc_lstm_cell_fwd_idx(const float* gx_all, const int* rows, const float* gh, const float* c_prev, const float* h_prev,
                           const float* active, float* h, float* c, float* gates_act, int N, int D, svpc_stream_t stream);
int svpc_lstm_cell_bwd_seq(const float* dh_out, const float* dh_rec, const float* dc, const float* gates_act, const float* c_prev,
                           const float* active, float* dgates, float* dc_prev, float* dh_prev, int N, int D, svpc_stream_t stream);
/* both directions of the BiLSTM at one time step in one launch: every argument is a HOST array of 2 device pointers
 * (direction 0 = forward in time, 1 = reverse); `active` is shared */
int svpc_lstm_pair_fwd(const float* const* gx, const int* const* rows, const float* const* gh, const float* const* c_prev,
                       const float* const* h_prev, const float* active, float* const* h, float* const* c, float* const* gates, int N, int D,
                       svpc_stream_t stream);
/* one time step of both directions with the recurrent projection inside: gates = gx[rows] + h_prev·W_hhᵀ (bf16 MFMA operands, fp32
 * accumulate) and the cell in ONE launch — a workgroup owns 8 hidden units (their i|f|g|o rows of W_hh), so no (N, 4D) buffer goes
 * through HBM between a GEMM and a cell launch.  D % 16 == 0.  Arguments as svpc_lstm_pair_fwd (w_hh[z]: (4D, D) row-major). */
int svpc_lstm_pair_step_fwd(const float* const* h_prev, const float* const* c_prev, const float* const* w_hh, const float* const* gx,
                            const int* const* rows, const float* active, float* const* h, float* const* c, float* const* gates, int N,
                            int D, svpc_stream_t stream);
int svpc_lstm_pair_step_fwd_x3(const float* const* h_prev, const float* const* c_prev, const float* const* w_hh, const float* const* gx,
                               const int* const* rows, const float* active, float* const* h, float* const* c, float* const* gates, int N,
                               int D, svpc_stream_t stream);   /* the same with bf16x3 products */
int svpc_lstm_pair_bwd(const float* const* dh_out, const float* const* dh_rec, const float* const* dc, const float* const* gates,
                       const float* const* c_prev, const float* active, float* const* dgates, float* const* dc_prev,
                       float* const* dh_prev, int N, int D, svpc_stream_t stream);
/* the same when the recurrent dgrad dgates·W_hh of the previous time step was computed in n_parts k-parts (more workgroups pulling
 * the weight): dh_parts[z] = n_parts slabs of N·D floats, added to dh_rec in part order */
int svpc_lstm_pair_bwd_parts(const float* const* dh_out, const float* const* dh_rec, const float* const* dh_parts, int n_parts,
                             const float* const* dc, const float* const* gates, const float* const* c_prev, const float* active,
                             float* const* dgates, float* const* dc_prev, float* const* dh_prev, int N, int D, svpc_stream_t stream);
/* greedy decoding step: argmax with the UNK column suppressed + OOV→UNK remap, src/translator.py:104-112 */
int svpc_greedy_pick(const float* scores, int ld, const int* row_c, const int* row_x, int n_sent, int lt, int pos, int unk,
                     int* next_ext, int* next_model, svpc_stream_t stream);
/* … and the picked ids also stored as column `col` of the sentence-major (n_sent, ld_out) id matrices the decoding loop keeps
 * (text_out: model-side ids, ext_out: extended ids; src/translator.py:96-99 writes them at the top of the next iteration) */
int svpc_greedy_pick_append(const float* scores, int ld, const int* row_c, const int* row_x, int n_sent, int lt, int pos, int unk,
                            int* next_ext, int* next_model, int* text_out, int* ext_out, int ld_out, int col, svpc_stream_t stream);
/* beam-search decoding step (src/translator.py:194-203 accepts `use_beam`; src/test.py:207-209 defines --use_beam / --beam_size): one
 * workgroup per sentence over its `beam` hypothesis rows r = t·beam + h of `scores` (row r: its first row_c[r] columns, the last row_x[r] of
 * them copied OOV words).  logits == 0: scores are probabilities p, step score log p (p <= 0: −inf); logits != 0: step score = logit − the
 * log-sum-exp of the row.  The UNK column is not a candidate.  Candidates rank by higher cum_parent + step, then higher raw value, then
 * lower parent·C + column; a finished hypothesis offers only itself (token pad, step 0).  In place: cum, finished (a child is finished once
 * its extended id is eos).  Out: parent (global parent row), next_ext / next_model (OOV → unk on the model side), and the ping-pong tables
 * (T·beam, ld_tok): text / ext ids and the KV-cache ancestry rows_out[r][j] = rows_in[parent][j] for j <= pos, rows_out[r][pos + 1] =
 * r·slot_rows + pos + 1 (the hypothesis's own cache slot).  No host synchronisation, fixed buffers: graph-capture safe. */
int svpc_beam_step(const float* scores, int ld, const int* row_c, const int* row_x, int n_sent, int beam, int pos, int logits, int unk,
                   int eos, int pad, int slot_rows, float* cum, int* finished, const int* text_in, const int* ext_in, const int* rows_in,
                   int* text_out, int* ext_out, int* rows_out, int ld_tok, int* parent, int* next_ext, int* next_model, svpc_stream_t stream);
/* end of the beam decode: per sentence the hypothesis with the highest cum (ties: the lowest index), its first lt ids of `ext`
 * ((n_sent·beam, ld_tok)) into best_ids ((n_sent, lt)) and its cum into best_score */
int svpc_beam_finalize(const float* cum, const int* ext, int ld_tok, int n_sent, int beam, int lt, int* best_ids, float* best_score,
                       svpc_stream_t stream);
/* svpc_beam_step with the decoding controls of the reference's OpenNMT-derived decoder lineage (min_length, block_ngram_repeat,
 * exclusion_tokens, length_penalty; src/train.py:548 and src/test.py:209 parse --n_best).  All off (0 / NULL) it is svpc_beam_step.
 * min_len m: eos is not a candidate while pos + 1 <= m.  ngram n > 0 (needs ld_tok <= 64): candidate (h, w) is skipped when the gram
 * (ext_in[h][pos + 2 − n … pos], w) already occurs in ext_in[h][1 … pos] and none of its ids is set in excl (a bitmap of excl_v ids; ids
 * >= excl_v, copied OOV words, are never excluded).  Skipped columns stay in the log-sum-exp of logits mode.  lp (NULL: none) is a length
 * penalty table of ld_tok doubles: candidates rank by (double)cum / lp[len], then the raw value, then the flat index; len (in place,
 * (T·beam,), needed with lp) is pos + 1 for a live parent's child and kept by a finished one. */
int svpc_beam_step_ctl(const float* scores, int ld, const int* row_c, const int* row_x, int n_sent, int beam, int pos, int logits, int unk,
                       int eos, int pad, int slot_rows, float* cum, int* finished, const int* text_in, const int* ext_in, const int* rows_in,
                       int* text_out, int* ext_out, int* rows_out, int ld_tok, int* parent, int* next_ext, int* next_model, int min_len,
                       int ngram, const unsigned* excl, int excl_v, const double* lp, int* len, svpc_stream_t stream);
/* svpc_beam_step_ctl with paragraph-scope n-gram blocking (ngram n >= 1, ld_tok <= 64, rows of at most 4096 columns): candidate (h, w) is
 * also skipped when the gram (ext_in[h][pos + 2 − n … pos], w) equals n consecutive words of an earlier sentence's caption and none of its
 * ids is set in excl.  Those captions are rows of `hist` ((rows, ld_tok) int32 extended ids, the decode's top-1 matrix): sentence t of the
 * step reads rows hist_desc[2t] … hist_desc[2t] + hist_desc[2t + 1] − 1.  The words of a row are its ids at positions 1 … L (position
 * L + 1: its first eos or pad, else L = ld_tok − 1), bos excepted; no gram spans two rows.  With every history empty it is
 * svpc_beam_step_ctl. */
int svpc_beam_step_para(const float* scores, int ld, const int* row_c, const int* row_x, int n_sent, int beam, int pos, int logits, int unk,
                        int eos, int pad, int slot_rows, float* cum, int* finished, const int* text_in, const int* ext_in, const int* rows_in,
                        int* text_out, int* ext_out, int* rows_out, int ld_tok, int* parent, int* next_ext, int* next_model, int min_len,
                        int ngram, const unsigned* excl, int excl_v, const double* lp, int* len, const int* hist, const int* hist_desc,
                        int bos, svpc_stream_t stream);
/* diverse (group) beam search (Vijayakumar et al. 2016, arXiv 1610.02424; Hamming diversity): svpc_beam_step_ctl over `beam` rows per
 * sentence that are `groups` groups of beam / groups rows (groups divides beam), row g·Bg + j hypothesis j of group g.  The groups pick in
 * order; a child (h, c) of group g pays pen[n], n the rows of groups 0 … g − 1 whose live pick at this step is c (the pad of a finished
 * parent and fill rows are not counted, eos is).  cum (in place) stays the model's sum; aug (in place, (T·beam,)) is the selection score:
 * aug' = fp32(fp32(aug_h + step) − pen[n]), and a group's candidates — those of its own rows — rank by (double)aug' / lp[len], then the raw
 * value, then the flat index h·C + c (h = 0 … beam − 1).  pen: beam floats, pen[n] = fp32(fp32(strength)·n), built on the host.  len is
 * required.  groups == 1 with aug == cum is svpc_beam_step_ctl. */
int svpc_beam_step_groups(const float* scores, int ld, const int* row_c, const int* row_x, int n_sent, int beam, int pos, int logits, int unk,
                          int eos, int pad, int slot_rows, float* cum, int* finished, const int* text_in, const int* ext_in, const int* rows_in,
                          int* text_out, int* ext_out, int* rows_out, int ld_tok, int* parent, int* next_ext, int* next_model, int min_len,
                          int ngram, const unsigned* excl, int excl_v, const double* lp, int* len, int groups, const float* pen, float* aug,
                          svpc_stream_t stream);
/* lexically constrained beam search (Post & Vilar 2018, dynamic beam allocation; fairseq's unordered --constraints): svpc_beam_step_ctl
 * whose sentences each have up to 4 phrases of 1 … 4 extended ids that a caption must contain.  cons: (n_sent, 4, 4) int32, a phrase the
 * leading non-negative ids of its row (the rest −1), a sentence's constraints its leading non-empty rows.  cstate ((T·beam,) int32, in
 * place, start 0): bits 0–3 one bit per constraint met, bits 4–6 cur + 1 (0: no phrase in progress), bits 8–10 off, the ids of phrase cur
 * matched so far.  A picked word c of an unfinished parent: cur >= 0 and c == phrase[cur][off] → off += 1 (a complete phrase sets its bit
 * and clears cur, off); otherwise the progress is dropped and the lowest unmet phrase starting with c starts (length 1: is met).  A
 * finished parent keeps its state, a fill row gets 0; bank n = Σ len of the met phrases + off.  (Not a string matcher: phrase `a a b` is
 * not completed by the text `a a a b`.)  Candidates of an unfinished row: the allowed columns of svpc_beam_step_ctl, eos also skipped
 * while a constraint is unmet; of these its top-beam by (raw, column) and its forced columns (phrase[cur][off], or without progress the
 * first ids of all unmet phrases) whose child has cum' > −inf.  Live candidates (cum' finite) rank inside their bank by
 * svpc_beam_step_ctl's order; the rows are filled in ascending (rank in bank, −bank), dead candidates last in svpc_beam_step_ctl's
 * order.  cum stays the model's sum; len is required.  With no constraints it is svpc_beam_step_ctl bit for bit. */
int svpc_beam_step_cons(const float* scores, int ld, const int* row_c, const int* row_x, int n_sent, int beam, int pos, int logits, int unk,
                        int eos, int pad, int slot_rows, float* cum, int* finished, const int* text_in, const int* ext_in, const int* rows_in,
                        int* text_out, int* ext_out, int* rows_out, int ld_tok, int* parent, int* next_ext, int* next_model, int min_len,
                        int ngram, const unsigned* excl, int excl_v, const double* lp, int* len, const int* cons, int* cstate,
                        svpc_stream_t stream);
/* end of the constrained beam decode: svpc_beam_finalize_nbest in the order: rows with cum = −inf last (by beam index); above them more
 * constraints met (bits 0–3 of cstate) first, then the higher (double)cum / lp[len], then the lower beam index.  best_met ((n_sent,
 * n_best)): the rows' met masks. */
int svpc_beam_finalize_cons(const float* cum, const int* len, const double* lp, const int* ext, const int* cstate, int ld_tok, int n_sent,
                            int beam, int lt, int n_best, int* best_ids, float* best_score, int* best_len, int* best_met,
                            svpc_stream_t stream);
/* end of the beam decode, n-best: per sentence its n_best (1 … beam) hypotheses in order of (double)cum / lp[len] (lp NULL: cum), ties to
 * the lower beam index; their first lt ids of `ext` into best_ids ((n_sent, n_best, lt)), cum into best_score and len into best_len
 * ((n_sent, n_best); best_len may be NULL, len may be NULL without lp).  n_best = 1 without lp is svpc_beam_finalize. */
int svpc_beam_finalize_nbest(const float* cum, const int* len, const double* lp, const int* ext, int ld_tok, int n_sent, int beam, int lt,
                             int n_best, int* best_ids, float* best_score, int* best_len, svpc_stream_t stream);
/* stochastic beam search (Kool, van Hoof and Welling 2019, arXiv 1903.06059): svpc_beam_step's launch shape, tables and step score over
 * `beam` rows per sentence, selecting by Gumbel-perturbed log-probabilities, so that a sentence's rows are a sample without replacement
 * from the model's sequence distribution, in the order drawn.  In place, (n_sent·beam,): cum (fp32, the model's sum, as svpc_beam_step's),
 * phi (fp64, the log-probability of the row's sequence under the tempered, renormalised model), gkey (fp64, the perturbed log-probability
 * G), finished, len; a dead row is finished with G = −inf; start: row 0 of a sentence (0, 0, 0, live), the others dead.  A live row h
 * (global row r): candidates are the columns c < row_c[r] <= max_c <= 4096, c != unk, with a finite step score s_c, eos excluded while
 * pos + 1 <= min_len; z_c = (double)s_c / temp, L their log-sum-exp, phi_c = phi_h + (z_c − L), g_c = phi_c − log(−log u), u =
 * (svpc_hash32(*seed, pos, r·4096 + c) + 0.5)·2^-32; the row's first `beam` candidates by higher g, then lower c, are short-listed, Z the
 * first one's g, and get G'_c = G_h − max(v, 0) − log1p(exp(−|v|)), v = G_h − g_c + log1p(−exp(g_c − Z)).  A finished row with finite G
 * offers itself (pad, step 0, G' = g = G_h, flat index h·4096 + pad), a dead row and a live row without candidates nothing.  The new rows
 * 0 … beam − 1 are the sentence's first candidates by higher G', then higher g, then lower flat index h·4096 + c: cum = fp32(cum_h + s_c),
 * phi = phi_c, G = G'_c, len = pos + 1, finished on eos; leftover slots are dead rows (pad, cum = phi = G = −inf, finished, len = pos + 1,
 * parent their own slot).  Out as svpc_beam_step's.  *seed is read on the device: graph-capture safe. */
int svpc_beam_step_gumbel(const float* scores, int ld, const int* row_c, const int* row_x, int n_sent, int beam, int pos, int logits, int unk,
                          int eos, int pad, int slot_rows, float* cum, int* finished, const int* text_in, const int* ext_in,
                          const int* rows_in, int* text_out, int* ext_out, int* rows_out, int ld_tok, int* parent, int* next_ext,
                          int* next_model, double temp, int min_len, const long long* seed, double* phi, double* gkey, int* len, int max_c,
                          svpc_stream_t stream);
/* contrastive search (Su et al. 2022; HuggingFace generate(penalty_alpha, top_k)): svpc_beam_step's launch shape, score rows and ping-pong
 * tables over `k` candidate rows per sentence, with the state per SENTENCE: ids / pen ((n_sent, ld_tok): the committed extended ids and the
 * winners' penalties), cum (fp32), len, finished ((n_sent,)), hist ((n_sent, ld_tok, d) fp32: the committed positions' hidden states) and
 * hist_n2 ((n_sent, ld_tok) fp64: their squared norms).  Called AFTER the decoder pass at position pos, whose row r = t·k + h carries one
 * candidate word for position pos (extended id ext_in[r][pos]) with cand_p[r] (its probability; 0: dead) and cand_score[r] (its step score),
 * and whose last-layer output is hidden[r] (d floats, row stride ld_h).  penalty_r = max over j < pos of cos(hidden[r], hist[t][j]) (fp64
 * dots and norms in a fixed order; 0 at pos 0 and when a norm is 0); score_r = (1 − alpha)·p_r − alpha·penalty_r; the winner is the live row
 * with the highest score, ties to the lowest row → winner[t] (−1: none).  Commit: ids[t][pos] = its id, cum[t] += its step score, len[t] =
 * pos, pen[t][pos], hist[t][pos] and hist_n2[t][pos]; eos finishes the sentence.  Expansion (pos + 1 < ld_tok, not finished): the top k
 * columns c < row_c <= max_c <= 4096 of the winner's score row by higher raw value, then lower column, without unk and without eos while
 * pos + 1 <= min_len, become the k rows' candidates at pos + 1: p the raw value (<= 0: 0), in logits mode fp32(exp(raw − lse)); a column
 * with p = 0 or a missing one is dead (pad, p 0, step score −inf); every child takes the winner's token and ancestry rows for positions <=
 * pos and its own cache slot at pos + 1, out as svpc_beam_step's.  A finished sentence writes pad children and nothing else; a sentence
 * without a live row finishes with pad and cum = −inf.  scores may be NULL at pos + 1 == ld_tok (no expansion).  Everything travels by
 * value: graph-capture safe. */
int svpc_contrastive_step(const float* scores, int ld, const int* row_c, const int* row_x, int n_sent, int k, int pos, int logits, int unk,
                          int eos, int pad, int slot_rows, const float* hidden, int ld_h, int d, double alpha, int min_len, int max_c,
                          float* cand_p, float* cand_score, const int* text_in, const int* ext_in, const int* rows_in, int* text_out,
                          int* ext_out, int* rows_out, int ld_tok, int* parent, int* next_ext, int* next_model, int* ids, float* cum,
                          int* len, float* pen, int* finished, float* hist, double* hist_n2, int* winner, svpc_stream_t stream);
/* random-sampling decoding step (the random-sampling strategy of the reference's OpenNMT decode-strategy lineage: random_sampling_temp,
 * random_sampling_topk, random_sampling_topp): one wave per sample row r of `scores` (n_rows rows; row r: its first row_c[r] <= max_c <= 4096
 * columns, the last row_x[r] of them copied OOV words).  Step scores as svpc_beam_step's (logits == 0: log p; logits != 0: logit − the
 * log-sum-exp of the row without unk).  Candidates: columns != unk with a finite step score, eos excluded while pos + 1 <= min_len, in order
 * of higher raw value then lower column; top-k (topk > 0) keeps the first topk, z = (double)step / temp, top-p (0 < topp < 1) keeps the
 * shortest prefix holding topp of the mass exp(z − z_first); the pick is the Gumbel-max over what is kept, with u = (svpc_hash32(*seed, pos,
 * r·4096 + c) + 0.5)·2^-32, ties to the lower column.  In place: cum (fp32 cum + step), finished (pick eos), len (pos + 1); a finished row
 * takes pad (step 0, len kept), a row without candidates pad, cum −inf, finished.  Out: next_ext / next_model (OOV → unk on the model side)
 * and column pos + 1 of the (n_rows, ld_tok) id matrices text_out / ext_out.  *seed is read on the device: graph-capture safe. */
int svpc_sample_step(const float* scores, int ld, const int* row_c, const int* row_x, int n_rows, int max_c, int pos, int logits, int unk,
                     int eos, int pad, double temp, int topk, double topp, int min_len, const long long* seed, float* cum, int* finished,
                     int* len, int* text_out, int* ext_out, int ld_tok, int* next_ext, int* next_model, svpc_stream_t stream);
/* svpc_sample_step with four further truncation stages between top-p and the draw, in this order, each off at 0 and each over the
 * distribution renormalised over the survivors of the stage before it (first = the first survivor in candidate order, w = exp(z − z_first),
 * q = w / Σ w, ln q = (z − z_first) − ln Σ w, all fp64): min_p in [0, 1) keeps w >= min_p; typical_p in [0, 1] (1: off) keeps the columns
 * with |−ln q − H| <= d*, H the entropy, d* the smallest such distance whose columns hold typical_p of the mass (equal distances stay or go
 * together; the mode may go); epsilon in [0, 1) keeps q >= epsilon; eta in [0, 1) keeps q >= min(eta, sqrt(eta)·exp(−H)); min-p, epsilon
 * and eta always keep the first survivor.  The draw (same z, same hash index, same tie rule) is over what is left; cum adds the
 * untruncated step score.  kept_out (n_rows, may be NULL): the size of the final set of each live row, 0 for a finished or empty row.
 * All four at 0: the results of svpc_sample_step bit for bit. */
int svpc_sample_step_trunc(const float* scores, int ld, const int* row_c, const int* row_x, int n_rows, int max_c, int pos, int logits,
                           int unk, int eos, int pad, double temp, int topk, double topp, int min_len, const long long* seed, float* cum,
                           int* finished, int* len, int* text_out, int* ext_out, int ld_tok, int* next_ext, int* next_model, double min_p,
                           double typical_p, double epsilon, double eta, int* kept_out, svpc_stream_t stream);
/* the seed of one sampling decode, on the device: src = (fixed, value); fixed != 0: *used = value; otherwise *used is drawn from the
 * decode's seed word *word, which advances (consecutive replays of one captured decode draw different streams) */
int svpc_sample_seed(const long long* src, long long* word, long long* used, svpc_stream_t stream);
/* ---- ensemble decoding (OpenNMT's EnsembleModel / avg_raw_probs; the reference vendored its decode strategies without it): n_members
 * (1..8) models deliver one fp32 score matrix each for the same n_rows hypothesis rows, and the step kernels above see ONE matrix.
 * scores / ld / weights are HOST arrays of n_members device pointers, leading dimensions and fp64 weights (finite, >= 0, not all 0; the
 * caller normalises them to sum 1); they are copied into the kernel's by-value arguments, so there is no table in device memory and a
 * captured decode replays the launch unchanged.  A member with weight 0 is never read.  Row r has C = row_c[r / rows_per] <= max_c columns
 * (max_c 1..4096, within every ld and ld_out).  Member probability p (fp64): logits == 0: raw > 0 ? raw : 0; logits != 0: exp(raw − lse),
 * lse the log-sum-exp of the member row's columns c < C, c != unk, with p[unk] = 0 and a row without a finite logit contributing 0.
 * rule 0 ("prob"): out = fp32(sum_m w_m·p_m), terms in ascending m, multiply and add rounded separately; rule 1 ("logprob"): out =
 * fp32(exp(sum_m w_m·log p_m)), 0 once a counted member has p = 0, not renormalised.  Columns C <= c < ld_out are written 0.  out is a
 * PROBABILITY matrix in both modes: the step kernels take it with logits = 0.  n_rows == 0 returns 0. */
int svpc_ensemble_combine(const float* const* scores, const int* ld, const double* weights, int n_members, const int* row_c, int rows_per,
                          int n_rows, int max_c, int logits, int unk, int rule, float* out, int ld_out, svpc_stream_t stream);
/* ---- contrastive decoding (Li et al. 2023; O'Brien & Lewis 2023; with the amateur the same model without the video: visual contrastive
 * decoding, Leng et al. 2024): an expert's score matrix held against an amateur's, for the same n_rows hypothesis rows.  expert / amateur:
 * fp32 matrices with leading dimensions ld_e / ld_a, probabilities (logits == 0) or raw logits (logits != 0).  Row r has
 * C = row_c[r / rows_per] <= max_c columns (max_c 1..4096, within ld_e, ld_a and ld_out).  Coefficients fp64: we > 0, wa >= 0, alpha in
 * [0, 1], log_alpha = log(alpha) computed on the host (−inf for alpha = 0).  unk is never a candidate: it is left out of every maximum,
 * head and sum in BOTH score modes, and out[unk] = 0.  The rule, one row at a time:
 *   1. member log-probabilities, fp64, for c < C, c != unk: probability mode p = raw > 0 ? (double)raw : 0 and l = log p (−inf at 0);
 *      logits mode l = (double)raw − lse, lse as svpc_ensemble_combine defines it; a member row without a finite non-unk logit is dead:
 *      l = −inf everywhere;
 *   2. dead expert row (no column with l_e > −inf): the whole output row is 0;
 *   3. head H: probability mode p_e,c > 0 and p_e,c >= alpha·p_e,top (one rounded fp64 product); logits mode raw_e,c finite and
 *      (double)raw_e,c − (double)raw_e,top >= log_alpha; no row reduction other than an exact maximum: bit-reproducible;
 *   4. amateur term la_c = max(l_a,c, L0), L0 = log(1e-30) = -69.07755278982137 (a zero amateur probability and a dead amateur row
 *      without an infinity); with wa == 0 the amateur matrix is never read (amateur may be null);
 *   5. score s_c = we·l_e,c − wa·la_c, the two products and the difference each rounded, never contracted;
 *   6. normalise: m = max_H s, Z = sum_H exp(s_c − m), out_c = fp32(exp((s_c − m) − log Z)) for c in H; a head of one column gives
 *      exactly 1.0;
 *   7. columns outside H, unk, and C <= c < ld_out are 0.
 * out is a distribution over the head: the step kernels take it with logits = 0.  n_rows == 0 returns 0. */
int svpc_contrast_combine(const float* expert, int ld_e, const float* amateur, int ld_a, double we, double wa, double alpha,
                          double log_alpha, const int* row_c, int rows_per, int n_rows, int max_c, int logits, int unk, float* out,
                          int ld_out, svpc_stream_t stream);
/* ---- evaluation tail of a decode: the caption the reference submits and its repetition / diversity counts, on the device
 *      (recursive_caption_dataset.py:472-500 convert_ids_to_sentence, src/translate.py:27-42 remove_dup, densevid_eval/evaluateRepetition.py,
 *      evaluateCaptionsDiversity.py:219-282, get_caption_stat.py; the reference copies every sentence to the host, translate.py:81-82).
 * svpc_caption_clean: id row r = the lt ids at ids + (r·row_stride + row_pick)·ld (int64 when ids64, else int32; row_stride / row_pick
 * take row k of (T, K, Lt) n-best / sample outputs), lt <= 64.  Clean caption: the ids without pad and ignore, without the first of those,
 * up to (not including) the first eos, runs of one id collapsed to one (remove_dup != 0).  Out: words (n_rows, lt) int32, the caption
 * left-aligned and pad-filled, and len (n_rows,) int32 (0 … lt − 1). */
int svpc_caption_clean(const void* ids, int ids64, long long ld, int row_stride, int row_pick, int n_rows, int lt, long long pad,
                       long long eos, long long ignore, int remove_dup, int* words, int* len, svpc_stream_t stream);
/* per video b (rows vid_off[b] … vid_off[b + 1] − 1 of words / len, at most 4096 / lt rows — the host checks; a larger video's row is −1):
 * its repetition words are each clean caption without a final `period` word and without any `comma` word (INT_MIN: no such id); an n-gram is
 * n consecutive repetition words of one caption.  counts (n_vid, 12) int32 = total_1..4 (n-grams), distinct_1..4 (different ones, compared
 * id by id), n_sen, n_words (clean words, before the punctuation rule), n_empty (clean captions of length 0), n_copied (clean words >= vocab).
 * vocab_bits (or NULL): bit w of the bitmap is set (atomic OR) for every clean word 0 <= w < vocab. */
int svpc_caption_ngram_counts(const int* words, const int* len, const int* vid_off, int n_vid, int lt, int period, int comma, int vocab,
                              int* counts, unsigned* vocab_bits, svpc_stream_t stream);
/* acc[0..12] += Σ_b (re_1..4, div_1..4, 1, n_sen, n_words, n_empty, n_copied) over the n_vid rows of counts, re_n = (total_n − distinct_n) /
 * total_n (0 when total_n = 0), div_n = distinct_n / total_1 (0 when total_1 = 0); fp64, summed in a fixed order (deterministic). */
int svpc_decode_metric_accum(const int* counts, int n_vid, double* acc, svpc_stream_t stream);
/* ---- ingredient-prediction recall / precision / F1 of clean captions (src/calculate_ingredient_f1.py:6-59), on the device.  The
 *      reference's string rule (`ingredient in sentence`, then `word in all_ingredient_dict`) is carried by bit tables the host compiles
 *      (svpc_amd/ingredients.py): pred (n_pred, pred_ld) — row p, bit i: vocabulary word i satisfies predicate p (contains / ends with /
 *      equals / starts with a string); a_bits — vocabulary words in the global ingredient set.  words (n_rows, lt) / len as
 *      svpc_caption_clean writes them; vid_off (n_vid + 1) first rows of the videos; row_vs (n_rows, 2) = (video, step) of every row.
 *      vid (n_vid, 8) = {ing0, E <= 64, X <= 128 copied words, eq0, n_eq, gt0, n_gt, 0}: listed ingredient e of the video owns the pattern
 *      tokens ing_tok[ing0 + e] … ing_tok[ing0 + e + 1] − 1; token j = predicate row tok_row[j] for ids < vocab and the 128 bits
 *      tok_oov[4 j …] for the copied ids vocab … vocab + X − 1.  Ingredient e is mentioned when its tokens hold at consecutive positions.
 *      Extra words: positions whose id is none of eq_ids[eq0 … eq0 + n_eq − 1] (ids that spell a whole listed ingredient) and is in the
 *      set (a_bits, or the video's 128 bits oov_a[4 b …]).  Generated step s < n_gt is compared with ground-truth step g = gt0 + s:
 *      gt_mask (2 words per step, low first) its listed ingredients, gx_ids[gx_off[g] … gx_off[g + 1] − 1] the ids of its extra words,
 *      gt_len[g] the length of its list.  Out: masks (n_rows) int64, extra (n_rows) extra words, row_counts (n_rows, 3) = correct, generated
 *      list length, ground-truth list length (zeros for a step without ground truth), vid_counts (n_vid, 3) their sums per video;
 *      acc[0..2] (or NULL) += the three totals, 64-bit integer atomics: any sequence of calls gives the same bits. */
int svpc_caption_ingredients(const int* words, const int* len, int n_rows, int lt, const int* vid_off, const int* row_vs, int n_vid,
                             const unsigned* pred, int pred_ld, int n_pred, const unsigned* a_bits, int vocab, const int* vid,
                             const int* ing_tok, const int* tok_row, const unsigned* tok_oov, const int* eq_ids, const unsigned* oov_a,
                             const unsigned* gt_mask, const int* gt_len, const int* gx_off, const int* gx_ids, long long* masks, int* extra,
                             int* row_counts, int* vid_counts, unsigned long long* acc, svpc_stream_t stream);
/* ---- Bleu_1..4, ROUGE_L and CIDEr of clean captions against reference paragraphs (densevid_eval/para-evaluate.py:26-29, 71-84, 112-125 with
 *      Bleu(4) option `closest`, Rouge beta = 1.2, Cider() n = 4 sigma = 6; the definitions: DESIGN 11.6), on the device.  A token is an id
 *      1 … 65534 of the host's token lexicon (svpc_amd/caption_scores.py).  An n-gram (n <= 4) is the 64-bit key t0 | t1 << 16 | t2 << 32 |
 *      t3 << 48 of its ids, absent fields 0.  The gram -> idf table (tab_key, tab_idf; tab_cap a power of two; key 0 = empty slot; built on
 *      the host, only probed here) is open addressing with linear probing from slot (h ^ (h >> 32)) & (tab_cap - 1), h = key *
 *      0x9E3779B97F4A7C15 (mod 2^64); a gram absent from it has idf log_docs = ln(number of reference videos).
 *      vid (n_vid, 12) int32 = {n_ref <= 4, index of the video in the reference set, X <= 128 copied words, oov0, ref_off[4], ref_len[4]}.
 * svpc_caption_tokens: the token stream of video b's clean captions (rows vid_off[b] … vid_off[b + 1] - 1 of words / len as
 * svpc_caption_clean writes them, in order): word id w < vocab gives voc_tok[voc_off[w] … voc_off[w + 1] - 1], copied id vocab + x (x < X)
 * gives oov_tok[oov_off[oov0 + x] … oov_off[oov0 + x + 1] - 1], any other id nothing.  Out: tokens (n_vid, 1024) int32 (zero-filled past
 * the end) and tok_len (n_vid,) — -1 for a video over 1024 tokens (the host refuses what could get there). */
int svpc_caption_tokens(const int* words, const int* len, const int* vid_off, int n_vid, int lt, int vocab, const int* voc_off,
                        const int* voc_tok, int n_voc_tok, const int* vid, const int* oov_off, int n_oov_off, const int* oov_tok,
                        int n_oov_tok, int* tokens, int* tok_len, svpc_stream_t stream);
/* per video: reference r = the ref_len[r] <= 1024 16-bit tokens at ref_tok + ref_off[r] (n_ref_tok in all), ref_norm (n_vid, 4, 4) its
 * CIDEr norms per n (fp64, from the host), gauss[d] = exp(-d^2 / 72) for d = 0 … 1023.  counts (n_vid, 11) int32 = correct_1..4 (clipped
 * n-gram matches), guess_1..4 (max(0, testlen - n + 1)), testlen, reflen (closest reference length, ties to the shorter), the largest LCS;
 * scores (n_vid, 6) fp64 = the video's own Bleu_1..4, ROUGE_L, CIDEr; every fp64 sum in a fixed order (the same inputs give the same
 * bits).  seen (or NULL): seen[index of the video] = 1 (n_seen entries).  A video whose tok_len is -1: counts -1, scores 0. */
int svpc_caption_score_counts(const int* tokens, const int* tok_len, int n_vid, const int* vid, const double* ref_norm,
                              const unsigned short* ref_tok, long long n_ref_tok, const unsigned long long* tab_key, const double* tab_idf,
                              int tab_cap, double log_docs, const double* gauss, int* counts, double* scores, long long* seen, int n_seen,
                              svpc_stream_t stream);
/* acc_i[0..10] += sums of correct_1..4, guess_1..4, testlen, reflen and the number of videos (64-bit integers), acc_f[0..1] += sum of
 * ROUGE_L, sum of CIDEr over the n_vid rows (a thread's rows in index order, then a fixed tree: deterministic); rows of -1 are left out. */
int svpc_caption_score_accum(const int* counts, const double* scores, int n_vid, unsigned long long* acc_i, double* acc_f,
                             svpc_stream_t stream);
/* ---- consensus (minimum Bayes risk) selection among the K <= 16 decoded candidates of a group: candidate i's utility against
 *      candidate j is the six scores above with i as the hypothesis and j as the single reference, j's length and CIDEr norms computed on
 *      the device by the same formulas (ROUGE_L against an empty j is 0); tokens, gram keys and the gram -> idf table as above.
 * svpc_consensus_tokens: stream s = the clean rows first, first + stride, …, first + (rows - 1) * stride of words / len (n_rows rows, as
 * svpc_caption_clean writes them) with streams (n_streams, 4) int32 = {first, rows, stride, video}; the video's row of vid (n_vid, 12)
 * gives its copied words.  Out: tokens (n_streams, 1024) 16-bit (zero past the end), tok_len (n_streams,) — -1 over 1024 tokens. */
int svpc_consensus_tokens(const int* words, const int* len, long long n_rows, const int* streams, int n_streams, int lt, int vocab,
                          const int* voc_off, const int* voc_tok, int n_voc_tok, const int* vid, int n_vid, const int* oov_off, int n_oov_off,
                          const int* oov_tok, int n_oov_tok, unsigned short* tokens, int* tok_len, svpc_stream_t stream);
/* group g = the streams g * k … g * k + k - 1.  out (n_grp, k, k, 6) fp64: out[g][i][j] = Bleu_1..4, ROUGE_L, CIDEr of hypothesis i against
 * the reference j, for every ordered pair, i = j included; every fp64 sum in a fixed order (the same inputs give the same bits).  A pair
 * with a stream whose tok_len is -1: zeros.  work: n_grp * k * 4 doubles of the caller's (the candidates' squared norms between the two
 * launches: one workgroup per (group, hypothesis), then one thread per pair). */
int svpc_consensus_pair_scores(const unsigned short* tokens, const int* tok_len, int n_grp, int k, const unsigned long long* tab_key,
                               const double* tab_idf, int tab_cap, double log_docs, const double* gauss, double* out, double* work,
                               svpc_stream_t stream);
/* per group g (its sentences are the rows grp_off[g] … grp_off[g + 1] - 1 of the n_rows): expected[g][i] = sum over j != i (ascending) of
 * w_j * pair[g][i][j][col] / sum of w_j (0 when that is 0), fp64; w_j = 1, or with posterior != 0 exp(c_j - max c), c_j the fp64 sum over the
 * group's rows in order of scores (n_rows, k) fp32 (all weights 1 when the maximum is -inf); pick[g] = the arg max, ties to the lowest i.
 * With out_ids: for every row r of the group out_ids[r] = the lt ids of row pick of ids (n_rows, k, lt) (int64 when ids64, else int32),
 * row_pick[r] = pick, and out_scores[r] / out_len[r] (or NULL) the chosen entries of scores / lengths (n_rows, k). */
int svpc_consensus_pick(const double* pair, int n_grp, int k, int col, int posterior, const float* scores, const int* grp_off,
                        long long n_rows, const void* ids, int ids64, int lt, const long long* lengths, int* pick, double* expected,
                        long long* out_ids, long long* row_pick, float* out_scores, long long* out_len, svpc_stream_t stream);

/* ---- forced decoding: the decoder's scores of GIVEN captions (the GOLD score / gold perplexity of the reference decoder's
 *      OpenNMT lineage).  n_cap caption rows of lt positions, extended ids, position 0 BOS; the decoder side runs once over all positions,
 *      score row r·lt + i scores position p = i + 1 of caption r.  A caption ends finished at its first eos (len = p) or unfinished before
 *      its first pad / ignore (len = p − 1), else len = lt − 1. */
/* ids (n_cap, lt) int64 (ids_i64) or int32 -> model_ids (an id outside [0, vocab) is unk; pad after position len), mask (fp32, 1 on
 * positions 0 … len), tgt (the id of every position as a score column; −2 when it fits no int32), len, finished (n_cap,) */
int svpc_force_inputs(const void* ids, int ids_i64, int n_cap, int lt, int vocab, int unk, int eos, int pad, int ignore, int* model_ids,
                      float* mask, int* tgt, int* len, int* finished, svpc_stream_t stream);
/* one wave per score row (r, i), i < len[r]: scores (>= n_cap·lt rows of ld floats; row_c[r] <= max_c <= ld columns) — probabilities, or
 * logits when logits != 0.  Candidates: columns c < row_c[r], c != unk, in order of higher raw value then lower column.  Out, at
 * r·(lt − 1) + i: step = the step score of column w = tgt[r·lt + i + 1] as svpc_beam_step's (fp64, rounded once: log p, −inf for p <= 0; or
 * logit − the log-sum-exp of the row without unk), rank = the candidates ahead of w, top / top_step = the first candidate and its step
 * score.  w no candidate (unk, < 0, >= row_c[r]): rank −1, step −inf, or 0 when skip != 0.  Entries with i >= len[r] are not written. */
int svpc_force_score(const float* scores, int ld, const int* row_c, int max_c, const int* tgt, const int* len, int n_cap, int lt, int logits,
                     int unk, int skip, float* step, int* rank, int* top, float* top_step, svpc_stream_t stream);
/* per caption row: cum = fp32(cum + step) over i < len[r] in order, n_scored = the positions that contributed (all of them; with skip != 0
 * those whose target is a candidate); the entries i >= len[r] of step / rank / top / top_step become 0 / −1 / −1 / 0 */
int svpc_force_finish(const int* tgt, const int* len, const int* row_c, int n_cap, int lt, int unk, int skip, float* step, int* rank,
                      int* top, float* top_step, float* cum, int* n_scored, svpc_stream_t stream);
/* acc (9,) float64 += captions, positions scored, sum of cum and of n_scored over the captions with a finite cum, captions with a
 * non-finite cum, positions of rank 0, sum of rank and count of the ranked positions (rank >= 0, i < len[r]), finished captions — one
 * workgroup, fixed summation order */
int svpc_force_accum(const float* cum, const int* n_scored, const int* finished, const int* len, const int* rank, int n_cap, int lt,
                     double* acc, svpc_stream_t stream);

/* ---- sequence log-likelihood of given captions as a training loss (self-critical sequence training).  Layout and the
 *      caption's end as forced decoding above; tgt / len are svpc_force_inputs'; row_w (n_cap,) fp32 the captions' weights. */
/* step (n_cap, lt − 1) = svpc_force_score's step under unk = "bar" (0 past the end), cum (n_cap,) = fp32(cum + step) in position order,
 * barred (n_cap,) = 1 when a scored position's step is not finite, loss (1,) = fp32(−sum over the captions not barred of row_w·cum), the
 * products and sums in fp64 in a fixed order.  Three launches. */
int svpc_seq_nll_fwd(const float* scores, int ld, const int* row_c, int max_c, const int* tgt, const int* len, const float* row_w,
                     int n_cap, int lt, int logits, int unk, float* step, float* cum, int* barred, float* loss, svpc_stream_t stream);
/* dscores (n_cap·lt rows of ld_out floats) = d loss / d scores times the device scalar dl (1,), every element written: 0 from column
 * row_c[r] up, on the last position row of a caption, past its end and on every row of a barred caption; else −dl·row_w[r] / p at the target
 * column (probabilities) or dl·row_w[r]·(softmax without unk − [c = target]), 0 at unk (logits; the log-sum-exp in fp64). */
int svpc_seq_nll_bwd(const float* scores, int ld, const int* row_c, int max_c, const int* tgt, const int* len, const int* barred,
                     const float* row_w, const float* dl, int n_cap, int lt, int logits, int unk, float* dscores, int ld_out,
                     svpc_stream_t stream);
/* reward (n_vid, k) fp64, greedy (n_vid,) fp64 or NULL, row_vid (n_sent,) the sentences' videos -> advantage (n_vid, k) fp64 = reward −
 * baseline (rule 0: none; 1: greedy[b]; 2: the mean of the video's other k − 1 rewards, added in ascending order) and w (n_sent·k,) fp32 =
 * fp32(advantage[row_vid[t], k] / (n_vid·k)) at row t·k + k */
int svpc_scst_weights(const double* reward, const double* greedy, const int* row_vid, int n_vid, int k, int n_sent, int rule,
                      double* advantage, float* w, svpc_stream_t stream);

/* ---- unlikelihood training against repetition.  Layout, tgt / len / finished as the sequence log-likelihood above.  neg
 *      (n_cap, lt − 1, m) int32, 1 <= m <= 64, lists the negative columns of every scored position (−1: none); a listing counts when it is a
 *      candidate (0 <= c < row_c[r], c != unk) and i < len[r]; a column listed twice counts twice.  term = −log1p(−p_c) when 1 − p_c >= 1e-5,
 *      else −log 1e-5 with a zero gradient; p_c = the probability, or exp(logit − the log-sum-exp of the row without unk), in fp64. */
/* One wave per caption row, lt − 1 <= 64.  rule 0 ("token", neg has m = lt − 1): entry (r, i) lists the distinct columns among tgt[r, 1 … i]
 * in order of first occurrence without tgt[r, i + 1] and non-candidates, −1 after them and on the rows i >= len[r].  rule 1 ("ngram", m = 1,
 * 1 <= ngram <= 4): the words of row r are tgt[r, 1 … nw], nw = len[r] − finished[r]; a gram of ngram words inside one caption is a repeat
 * when an equal gram starts earlier in the caption or, with paragraph != 0, anywhere in row s·k + (r mod k) of a sentence s with
 * sent_first[r / k] <= s < r / k (sent_first (n_cap / k,): the first sentence of each sentence's video); entry (r, p − 1) = tgt[r, p] when
 * position p lies inside a repeat gram, else −1.  npen (n_cap,) = the counted negatives, nrep (n_cap,) = the repeat grams (0 under rule 0). */
int svpc_ul_negatives(const int* tgt, const int* len, const int* finished, const int* row_c, int n_cap, int lt, int unk, int rule, int ngram,
                      int paragraph, const int* sent_first, int k, int* neg, int* npen, int* nrep, svpc_stream_t stream);
/* step / cum / barred as svpc_seq_nll_fwd (the same bits); ulstep (n_cap, lt − 1) = fp32(sum of the row's terms) (0 past the end), ul
 * (n_cap,) = fp32(ul + ulstep) in position order, loss (1,) = fp32(−sum row_w·cum + sum row_u·ul) over the captions not barred, products and
 * sums in fp64 in svpc_seq_nll_fwd's order (row_u all 0: its bits).  Three launches. */
int svpc_seq_ul_fwd(const float* scores, int ld, const int* row_c, int max_c, const int* tgt, const int* len, const int* neg, int m,
                    const float* row_w, const float* row_u, int n_cap, int lt, int logits, int unk, float* step, float* ulstep, float* cum,
                    float* ul, int* barred, float* loss, svpc_stream_t stream);
/* dscores as svpc_seq_nll_bwd, every element written, with the unlikelihood term's gradient on the rows that are not zero: probabilities,
 * dl·row_u[r] / (1 − p_c) added at column c per counted, unclamped listing of c; logits, dl·row_u[r]·(a_c − A·p_c) added at every candidate
 * column, a_c = the sum of p_c / (1 − p_c) over those listings of c, A = the sum of a_c.  A row with dl·row_u[r] = 0 has svpc_seq_nll_bwd's bits. */
int svpc_seq_ul_bwd(const float* scores, int ld, const int* row_c, int max_c, const int* tgt, const int* len, const int* barred,
                    const int* neg, int m, const float* row_w, const float* row_u, const float* dl, int n_cap, int lt, int logits, int unk,
                    float* dscores, int ld_out, svpc_stream_t stream);

/* ---- knowledge distillation against a teacher's per-position distribution.  Layout, tgt / len as the sequence
 *      log-likelihood above.  scores (ld floats per row; logits != 0: raw logits) is the student's matrix, tq (ldq floats per row;
 *      teacher_logits != 0: raw logits) the teacher's over the same rows; max_c <= ld, ldq.  Over the candidates (c < row_c[r], c != unk),
 *      in fp64: q_c = raw > 0 ? raw : 0, or exp(raw − the teacher row's log-sum-exp without unk) (0 everywhere when that is not finite),
 *      never renormalised; l_c = log p_c, or raw − the student row's log-sum-exp; a column with q_c > 0 is clamped when p_c <= 0 or
 *      l_c < log 2^-100: its term is −q_c·log 2^-100 and its gradient 0. */
/* step / cum / barred as svpc_seq_nll_fwd (the same bits); kdstep (n_cap, lt − 1) = fp32(−sum q_c·l_c), hstep = fp32(−sum q_c·log q_c) over
 * the candidates with q_c > 0 (0 past the end), per lane the columns lane, lane + 64, … then the butterfly; kd / ent (n_cap,) their fp32
 * running sums in position order; loss (1,) = fp32(−sum row_w·cum + sum row_v·kd) over the captions not barred, products and sums in fp64
 * in svpc_seq_nll_fwd's order (row_v all 0: its bits).  Three launches. */
int svpc_seq_kd_fwd(const float* scores, int ld, const float* tq, int ldq, const int* row_c, int max_c, const int* tgt, const int* len,
                    const float* row_w, const float* row_v, int n_cap, int lt, int logits, int teacher_logits, int unk, float* step,
                    float* kdstep, float* hstep, float* cum, float* kd, float* ent, int* barred, float* loss, svpc_stream_t stream);
/* dscores as svpc_seq_nll_bwd, every element written, with the distillation term's gradient on the rows that are not zero: probabilities,
 * −dl·row_v[r]·q_c / p_c added at every unclamped column with q_c > 0; logits, dl·row_v[r]·(Q'·p_c − q'_c) added at every candidate column,
 * q' = q on the unclamped columns, Q' = sum q'.  The teacher gets no gradient.  A row with dl·row_v[r] = 0 has svpc_seq_nll_bwd's bits. */
int svpc_seq_kd_bwd(const float* scores, int ld, const float* tq, int ldq, const int* row_c, int max_c, const int* tgt, const int* len,
                    const int* barred, const float* row_w, const float* row_v, const float* dl, int n_cap, int lt, int logits,
                    int teacher_logits, int unk, float* dscores, int ld_out, svpc_stream_t stream);

/* ---- contrastive (SimCTG) training loss on the decoder's last-layer hidden states (Su et al. 2022), the training
 *      counterpart of svpc_contrastive_step.  hidden row r·lt + i (d floats, row stride ld_h) is h_i of caption row r; the caption's token
 *      set is positions 0 … len[r] (svpc_force_inputs' length, clamped into [0, lt − 1] on the device), n = len[r] + 1; 2 <= lt <= 32,
 *      1 <= d <= ld_h, lt·d·4 bytes <= 144 KB (the rows live in LDS), margin finite in (0, 2].  In fp64: q_i = |h_i|² and the dot
 *      products in svpc_contrastive_step's order (a q_i has hist_n2's bits); c_ij = h_i·h_j / (sqrt(q_i)·sqrt(q_j)), 0 when a norm is 0;
 *      m_ij = (margin − 1) + c_ij; the ordered pair (i, j), i != j, is active iff m_ij > 0. */
/* cl (n_cap,) = fp32(sum over i != j of max(0, m_ij) / (n(n − 1))), sim (n_cap,) = fp32(the mean of c_ij over i != j), nact (n_cap,) = the
 * active ordered pairs — all 0 for n < 2 —, q (n_cap, lt) fp64 = q_i (0 past the end), loss (1,) = fp32(sum of row_v·cl), products and
 * sums in fp64 in svpc_seq_nll_fwd's order.  No atomics: the same inputs give the same bits.  n_cap = 0: loss = 0.  Two launches. */
int svpc_seq_cl_fwd(const float* hidden, int ld_h, int d, const int* len, const float* row_v, int n_cap, int lt, double margin, float* cl,
                    float* sim, int* nact, double* q, float* loss, svpc_stream_t stream);
/* dh (n_cap·lt rows of ld_out >= d floats) = d loss / d hidden times the device scalar dl (1,), every element written:
 * dl·row_v[r]·(2 / (n(n − 1)))·(g_i − (g_i·u_i)·u_i) / sqrt(q_i) with u_i = h_i / sqrt(q_i) and g_i = the sum of u_j over the active pairs
 * (i, j), in fp64 and rounded once; 0 from column d up, for a zero row, past the caption's end and for n < 2.  The Gram matrix is
 * recomputed from the hidden rows (nothing else is saved).  n_cap = 0 returns 0.  One launch. */
int svpc_seq_cl_bwd(const float* hidden, int ld_h, int d, const int* len, const float* row_v, const float* dl, int n_cap, int lt,
                    double margin, float* dh, int ld_out, svpc_stream_t stream);

/* ---- minimum-risk and ranking training over a video's k candidate paragraphs.  Layout, tgt / len / row_w as the sequence
 *      log-likelihood above with n_cap = n_sent·k caption rows, row t·k + c; the sentences of video b are t = vid_off[b] … vid_off[b + 1] − 1
 *      (vid_off (n_vid + 1,) rises from 0 to n_sent); cost (n_vid, k) fp64.  In fp64, per video and candidate: s = the sum of cum over the
 *      video's sentences in order, n = max(1, the sum of len), z = s / n^length_beta (0 when a sentence of the candidate is barred); valid =
 *      no sentence barred and a finite cost; over the valid candidates, c ascending: q = exp(alpha·(z − max z)) / sum, risk = sum q·cost;
 *      pos = the valid candidates before this one by (cost, c); the pair (i, j), cost_i < cost_j, is active iff h = z_j − z_i + (pos_j −
 *      pos_i)·margin > 0, rank = the sum of h over the active pairs (j ascending inside i ascending); G = risk_weight·alpha·q_c·sum_c' q_c'·
 *      (cost_c − cost_c') + rank_weight·(active pairs with c as j − active pairs with c as i); an invalid candidate has q = 0, no pair, G = 0. */
/* step / cum / barred as svpc_seq_nll_fwd (the same bits); risk / rank (n_vid,), q / z (n_vid, k) fp64, valid (n_vid, k) int32, w_eff
 * (n_cap,) = fp32(row_w − G / (n_vid·n^length_beta)) — every element written —; loss (1,) = fp32(−sum row_w·cum over the captions not barred
 * + (risk_weight·sum risk + rank_weight·sum rank) / n_vid), each sum in svpc_seq_nll_fwd's order (both weights 0: its bits).  The gradient is
 * svpc_seq_nll_bwd under w_eff.  1 <= k <= 16; alpha, length_beta, margin and the weights finite and >= 0.  Four launches. */
int svpc_seq_risk_fwd(const float* scores, int ld, const int* row_c, int max_c, const int* tgt, const int* len, const float* row_w,
                      const double* cost, const int* vid_off, int n_vid, int n_sent, int k, int lt, int logits, int unk, double alpha,
                      double length_beta, double margin, double risk_weight, double rank_weight, float* step, float* cum, int* barred,
                      double* risk, double* rank, double* q, double* z, int* valid, float* w_eff, float* loss, svpc_stream_t stream);

/* ---- preference optimisation over a video's k candidate paragraphs against a frozen reference model (DPO, cDPO, IPO, SLiC's
 *      hinge, SimPO).  Layout, tgt / len / row_w / cost / vid_off as minimum-risk training above; ref_cum (n_cap,) fp32 the reference
 *      model's cum of the same captions, or NULL (reference-free: the bits of an all-zero ref_cum).  In fp64, per video and candidate:
 *      s / s_ref = the sums of cum / ref_cum over the video's sentences in order, n = max(1, the sum of len); valid = no sentence barred,
 *      every ref_cum finite and a finite cost; u = (s − s_ref) / n^length_beta (0 when invalid); pos = the valid candidates before this one
 *      by (cost, c); the pairs (i, j) of valid candidates: pairs 0 ("all") every cost_i < cost_j, 1 ("extremes") pos_i = 0 and pos_j = the
 *      valid count − 1 with cost_i < cost_j; d = u_i − u_j, h = beta·d − gamma; the pair's loss l: loss_type 0 (sigmoid) −(1 −
 *      label_smoothing)·ln s(h) − label_smoothing·ln s(−h) with ln s(x) = min(x, 0) − log1p(exp(−|x|)), 1 (hinge) max(0, 1 − h), 2 (ipo)
 *      (d − 1 / (2 beta))²; D = dl / dd; G = (pref_weight / P)·(the sum of D over the pairs with c as i − over the pairs with c as j), P the
 *      video's pairs; an invalid candidate stands in no pair and has G = 0. */
/* step / cum / barred are svpc_seq_nll_fwd's (it is called: the same bits); pref (n_vid,) fp64 = the mean of l over the video's pairs (per
 * i the sum over j ascending, then over i ascending), reward (n_vid, k) fp64 = beta·u, valid (n_vid, k) int32, n_pairs / n_correct (n_vid,)
 * int32 = P and the pairs with d > 0, margin (n_vid,) fp64 = the mean of beta·d over the pairs — pref and margin 0 with no pair —, w_eff
 * (n_cap,) = fp32(row_w − G / (n_vid·n^length_beta)) — every element written —; loss (1,) = fp32(−sum row_w·cum over the captions not barred
 * + pref_weight·sum pref / n_vid), each sum in svpc_seq_nll_fwd's order (pref_weight 0: its bits, the second term not added).  The gradient
 * is svpc_seq_nll_bwd under w_eff.  1 <= k <= 16; beta > 0; gamma, length_beta, pref_weight >= 0; 0 <= label_smoothing < 0.5 and 0 outside
 * loss_type 0; gamma 0 under loss_type 2; all finite.  Five launches. */
int svpc_seq_pref_fwd(const float* scores, int ld, const int* row_c, int max_c, const int* tgt, const int* len, const float* row_w,
                      const double* cost, const float* ref_cum, const int* vid_off, int n_vid, int n_sent, int k, int lt, int logits, int unk,
                      double beta, double gamma, double label_smoothing, double length_beta, double pref_weight, int loss_type, int pairs,
                      float* step, float* cum, int* barred, double* pref, double* reward, int* valid, int* n_pairs, int* n_correct,
                      double* margin, float* w_eff, float* loss, svpc_stream_t stream);

/* ---- clipped policy-gradient training over a video's k candidate paragraphs with a per-token KL against a frozen reference model
 *      (PPO's clipped surrogate in its group form GRPO; DAPO and Dr. GRPO are settings).  Layout, tgt / len / row_w / vid_off as
 *      preference optimisation above; adv (n_vid, k) fp64 the candidates' advantages; old_step / ref_step (n_cap, lt − 1) fp32 the behaviour
 *      policy's and the reference model's step scores of the same captions, or NULL (no old_step: the ratio is exactly 1; no ref_step: no KL
 *      term, kl_beta must be 0).  Per candidate: n = max(1, the sum of len over its sentences); valid = no sentence barred, a finite adv
 *      and every old_step / ref_step entry at its scored positions (i < len) finite.  In fp64, per scored position of a valid candidate:
 *      r = exp(step − old_step), A = adv; sur = min(r·A, clamp(r, 1 − clip_lo, 1 + clip_hi)·A), under dual_clip = c (0: off) and A < 0
 *      sur = max(sur, c·A), A = 0: sur = 0; active = sur is the unclipped r·A (strict comparisons: an r on a bound is active); d = ref_step −
 *      step, kl = exp(d) − d − 1; tok = −sur + kl_beta·kl; den = n_vid·k·n (norm 0, "sequence"), max(1, n_tok) (norm 1, "token") or n_vid·k
 *      (norm 2, "none"); g = −A·r·[active] + kl_beta·(1 − exp(d)). */
/* step / cum / barred are svpc_seq_nll_fwd's (it is called: the same bits); pos_w (n_cap, lt − 1) = fp32(row_w − g / den) at the scored
 * positions of a valid candidate, row_w at those of any other candidate, 0 past a caption's end; pg / kl (n_cap,) fp64 = the row's sums of
 * −sur and kl, n_clip (n_cap, 2) int32 = its positions clipped from above (r > 1 + clip_hi with A > 0, or r > c with A < 0) / from below
 * (r < 1 − clip_lo with A < 0), ratio_max (n_cap,) fp32 = its largest r (0 with none), valid (n_vid, k) int32, n_tok (1,) int32 = the
 * scored positions of all valid candidates; row_adv (n_cap,) fp64, row_n (n_cap,) int32 and row_tok (n_cap,) fp64 are the launches' own
 * tables (the row's candidate's A and n, 0 when it is not valid, and the row's sum of tok / den) — every element of every output written,
 * given a vid_off that covers the n_sent sentences —; loss (1,) = fp32(−sum row_w·cum over the captions not barred + sum row_tok), each
 * sum in svpc_seq_nll_fwd's order (kl_beta 0 and no valid candidate's A different from 0: its bits, the second term not added).  The
 * gradient is svpc_seq_pos_bwd under pos_w with dead = barred.  1 <= k <= 16; 0 <= clip_lo < 1; clip_hi, kl_beta >= 0; dual_clip 0 or
 * > 1; all finite.  No atomics.  Seven launches. */
int svpc_seq_pg_fwd(const float* scores, int ld, const int* row_c, int max_c, const int* tgt, const int* len, const float* row_w,
                    const double* adv, const float* old_step, const float* ref_step, const int* vid_off, int n_vid, int n_sent, int k, int lt,
                    int logits, int unk, double clip_lo, double clip_hi, double dual_clip, double kl_beta, int norm, float* step, float* cum,
                    int* barred, float* pos_w, double* pg, double* kl, int* n_clip, float* ratio_max, int* valid, int* n_tok, double* row_adv,
                    int* row_n, double* row_tok, float* loss, svpc_stream_t stream);
/* svpc_seq_nll_bwd with a weight per position: pos_w (n_cap, lt − 1) fp32 stands where row_w[r] stands, dead (n_cap,) int32 where barred
 * does (a dead caption's rows are zero).  One launch, every element of dscores written; with pos_w[r, :] = row_w[r] and dead = barred the
 * bits of svpc_seq_nll_bwd. */
int svpc_seq_pos_bwd(const float* scores, int ld, const int* row_c, int max_c, const int* tgt, const int* len, const int* dead,
                     const float* pos_w, const float* dl, int n_cap, int lt, int logits, int unk, float* dscores, int ld_out,
                     svpc_stream_t stream);
/* the candidates' advantages from their rewards, per video over its candidates with a finite reward in ascending c (the others get 0):
 * rule 0 (grpo) (r − mean) / (std + eps) with the population std, 1 (center) r − mean, 2 (rloo) r − the mean of the other finite rewards
 * (svpc_scst_weights' leave-one-out rule, unscaled).  Fewer than two finite rewards, or the largest equal to the smallest: every advantage
 * exactly 0 (a test, not arithmetic).  reward / adv (n_vid, k) fp64; 1 <= k <= 16; eps finite and >= 0.  One launch. */
int svpc_group_advantage(const double* reward, int n_vid, int k, int rule, double eps, double* adv, svpc_stream_t stream);

/* rows between storage kinds in one launch (data movement): dst[r] = convert(src[idx ? idx[r] : r]); kinds 0 fp32, 1 bf16, 2 split (two bf16
 * planes, the lo plane lo_* columns behind the hi plane).  Where rows join or leave an activation stream: the decoder's memory rows
 * (src/rtransformer/model.py:939-947) entering the split stream, its output leaving it (:1086), the [CLS] rows of the clip stream (:1062-1064). */
int svpc_rows_move(const void* src, int src_kind, int ld_src, int lo_src, const int* idx, void* dst, int dst_kind, int ld_dst, int lo_dst,
                   int R, int W, svpc_stream_t stream);
/* table[idx[r]] += rows[r], fp32 rows into a dense bf16 table (distinct idx): the gradient of gathered stream rows joins the stream's
 * gradient in place */
int svpc_scatter_add_rows_bf16(const float* rows, const int* idx, void* table, int ld_table, int R, int W, svpc_stream_t stream);
/* rows of two (R', W) fp32 tables through two index lists in one launch — the two directions of the BiLSTM (model.py:1022-1024):
 * mode 0: out[r] = a[ia[r]] + b[ib[r]];  mode 1: a[ia[r]] = b[ib[r]] = out[r];  mode 2: out[r] = a[ia[r]], out2[r] = b[ib[r]] */
int svpc_pair_rows(float* a, const int* ia, float* b, const int* ib, float* out, float* out2, int R, int W, int mode, svpc_stream_t stream);
/* out = bf16(a + b), a bf16 (NULL: a plain cast), b fp32: the two gradients of a stream tensor that is also consumed as fp32 rows (the
 * decoder's last rows: the LM head reads the stream, the pointer attention its fp32 copy — model.py:896-923) in one launch */
int svpc_add_cast_bf16(const void* a, const float* b, void* out, size_t n, svpc_stream_t stream);
/* out[r] = inv[r] >= 0 ? src[inv[r]] : 0 for r < n_rows — the rows of a packed (valid tokens only) tensor back in the padded layout the
 * reference's return values have (model.py:1105-1115), zeros at the pad positions; fp32 rows of W floats */
int svpc_rows_expand(const float* src, const int* inv, float* out, int n_rows, int W, svpc_stream_t stream);
int svpc_add(const float* a, const float* b, float* c, size_t n, svpc_stream_t stream);
int svpc_sum_all(const float* x, size_t n, float* out, float scale, svpc_stream_t stream);
int svpc_fill_from(float* x, size_t n, const float* v, svpc_stream_t stream);
int svpc_dropout_mask(float* out, size_t n, float p, unsigned site, const svpc_u64* seed, svpc_stream_t stream);
/* keep mask (1 / 0) of the dropout on the attention probabilities (model.py:213), (n_rows, max_k) with rows (sequence·H + head)·max_q +
 * query: the draw every attention kernel of the library makes for that element — one full hash per ROW, one add + xor-shift + 24-bit
 * multiply per element (the kernels are bound by vector-instruction issue).  For tests: the fp32 reference applies the kernels' own mask. */
int svpc_attn_dropout_mask(float* out, size_t n_rows, int max_k, float p, unsigned site, const svpc_u64* seed, svpc_stream_t stream);
int svpc_bump_seed(svpc_u64* seed, svpc_stream_t stream);

/* ---- fused training-step tail: clip_grad_norm_ train.py:141-142, BertAdam optimization.py:284-331, EMA :196-203.
 *      meta = device array of {float* p,g,m,v,ema; long long n; float wd; int pad; bf16* shadow (or NULL); bf16* shadow_lo (or NULL)};
 *      chunk tables built by the host.  shadow[i] = bf16(p[i]) is refreshed by the Adam kernel (operand storage of svpc_gemm_glds),
 *      shadow_lo[i] = bf16(p[i] - shadow[i]) likewise (second plane of svpc_gemm_p8x3's B operand). */
int svpc_opt_chunk(void);
int svpc_opt_meta_bytes(void);
int svpc_opt_step(const void* meta, const int* chunk_tid, const long long* chunk_start, const int* tensor_chunk_off, int n_tensors,
                  int n_chunks, float* partial, float* norms_sq, const float* hyper, svpc_stream_t stream);
int svpc_opt_zero_grad(const void* meta, const int* chunk_tid, const long long* chunk_start, int n_chunks, svpc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SVPC_HIP_H */
