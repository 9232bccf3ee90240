// bf16 GEMM with a K-STRIDED B operand on the 256×256 8-phase main loop of gemm_common.h ("p8t") — the input gradients (dgrad) of the
// bf16 activation streams' projections (reference: the backward of every nn.Linear of the clip encoder, src/rtransformer/model.py:195-197, :230, :259,
// :281, :551):
//
//   C[M,N] = ( A[M,K] · B[K,N] ) ⊙ act'(G[M,N]) + R[M,N]        A = dz (k-contiguous rows), B = the weight matrix W[K = out][N = in] as it is stored
//
// G (optional): what the forward of the activation in front of this projection's input kept (z for GELU / ReLU) — the dgrad applies the
// activation's backward in its epilogue; R (optional): the residual-path gradient a LayerNorm backward parked for this tensor.  Both bf16,
// C's layout.  Same contract as svpc_gemm_glds_rg's stream dgrads, which ran on the round-1 32-deep ping-pong kernel (≈0.26 of peak).
//
// A is staged as in gemm_p8.hip (st_16x32); the B half-tile image is the k-strided one — the weight rows as they lie in memory, read
// through ds_read_b64_tr_b16 (FragTr).
// Epilogue: fp32 sums through a wave-private LDS image in two 32-column passes, act'(G), + R, one rounding to bf16, 16-byte stores.
#include "gemm_common.h"

// one 32-column half of the wave's 128×64 block: fp32 sums → LDS image [128 rows][128 B] (16-byte chunk c of row r at c ^ (r & 7)) →
// a lane takes 8 consecutive columns of a row: ⊙ act'(G), + R, bf16, one 16-byte store
template <int GACT, bool HASR>
__device__ __forceinline__ void p8t_store_half(const floatx4 (&acc)[8][4], int jh, __bf16* __restrict__ C, const __bf16* __restrict__ G,
                                               const __bf16* __restrict__ R, int ldc, int row0, int col0, int M, int N, int lane,
                                               char* __restrict__ wl) {
    const int l15 = lane & 15, q = lane >> 4;
    const int c8 = lane & 3, cc = col0 + 32 * jh + 8 * c8, r0 = lane >> 2;      // 8 columns = chunks 2·c8, 2·c8 + 1
    const bool col_ok = cc + 8 <= N;
    // the G / R pieces of all 8 row groups are requested FIRST and land under the LDS staging: written as load → use → store per row
    // group the compiler has to keep every load behind the previous store (16 dependent round trips per tile: + 10 µs for R, + 18 for G)
    bf16x8 gv[GACT != ACT_NONE ? 8 : 1], rv[HASR ? 8 : 1];
    // an interior block (the common case) runs without per-row predicates: with them every store sits in its own exec-masked region
    // and the compiler drains the memory counter in front of each (8 store round trips per pass instead of 1)
    const bool interior = row0 + 128 <= M && col0 + 32 * jh + 32 <= N;      // wave-uniform
#define P8T_EPI_LOADS(GUARD)                                                                                               \
    _Pragma("unroll") for (int it = 0; it < 8; ++it) {                                                                     \
        const int r = it * 16 + r0;                                                                                        \
        if (!(GUARD) || (col_ok && row0 + r < M)) {                                                                        \
            const size_t o = (size_t)(row0 + r) * ldc + cc;                                                                \
            if (GACT != ACT_NONE) gv[it] = *reinterpret_cast<const bf16x8*>(G + o);                                        \
            if (HASR) rv[it] = *reinterpret_cast<const bf16x8*>(R + o);                                                    \
        }                                                                                                                  \
    }
#define P8T_EPI_STORES(GUARD)                                                                                              \
    _Pragma("unroll") for (int it = 0; it < 8; ++it) {                                                                     \
        const int r = it * 16 + r0;                                                                                        \
        const floatx4 v0 = *reinterpret_cast<const floatx4*>(wl + r * 128 + (((2 * c8) ^ (r & 7)) << 4));                  \
        const floatx4 v1 = *reinterpret_cast<const floatx4*>(wl + r * 128 + (((2 * c8 + 1) ^ (r & 7)) << 4));              \
        float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};                                             \
        if (!(GUARD) || (col_ok && row0 + r < M)) {                                                                        \
            const size_t o = (size_t)(row0 + r) * ldc + cc;                                                                \
            if (GACT != ACT_NONE) {                                                                                        \
                _Pragma("unroll") for (int j = 0; j < 8; ++j) v[j] *= act_grad_from_aux((float)gv[it][j], GACT, true);     \
            }                                                                                                              \
            if (HASR) {                                                                                                    \
                _Pragma("unroll") for (int j = 0; j < 8; ++j) v[j] += (float)rv[it][j];                                    \
            }                                                                                                              \
            bf16x8 ov;                                                                                                     \
            _Pragma("unroll") for (int j = 0; j < 8; ++j) ov[j] = (__bf16)v[j];                                            \
            *reinterpret_cast<bf16x8*>(C + o) = ov;                                                                        \
        }                                                                                                                  \
    }
    if (interior) { P8T_EPI_LOADS(false) } else { P8T_EPI_LOADS(true) }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int r = i * 16 + l15;
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const int c16 = jj * 4 + q;                 // 16-byte chunk (4 fp32 columns) of the 32-column row
            *reinterpret_cast<floatx4*>(wl + r * 128 + ((c16 ^ (r & 7)) << 4)) = acc[i][2 * jh + jj];
        }
    }
    if (interior) { P8T_EPI_STORES(false) } else { P8T_EPI_STORES(true) }
#undef P8T_EPI_LOADS
#undef P8T_EPI_STORES
}

struct P8tPolicy {
    static constexpr int MIN_NK = 1;
    static constexpr bool THREE_TERM = false;
    const __bf16* ga[2];
    const __bf16* gb[2][2];      // B: pieces 2·wave and 2·wave + 1 of both half-tiles; piece pi = k-rows 4·pi … 4·pi + 3, lane l ↔
    size_t stepB;                // (k-row 4·pi + (l >> 4), slot l & 15), holding logical chunk slot ^ tr_swizzle(k-row)
    int fr_off;
    FragTr tr;
    template <int W>
    __device__ __forceinline__ void stage(int t, char* dst) const {
        if (W < 2) {
            const __bf16* src = ga[W & 1] + (size_t)t * P8_BK;
            p8_dma2(src, src + 32, dst);
        } else {
            p8_dma2(gb[W & 1][0] + (size_t)t * stepB, gb[W & 1][1] + (size_t)t * stepB, dst);
        }
    }
    __device__ __forceinline__ bf16x8 frag_a(const char* img, int blk, int kb) const { return frag_rd(img, blk, kb, fr_off); }
    __device__ __forceinline__ bf16x8 frag_b(const char* img, int cb, int kb) const { return tr(img, cb, kb); }
    template <int PH>
    __device__ __forceinline__ void extra(const bf16x8 (&)[2][4]) const {}
};

template <int GACT, bool HASR>
__global__ __launch_bounds__(512) void gemm_p8t_kernel(const __bf16* __restrict__ A, int lda, const __bf16* __restrict__ B, int ldb,
                                                       __bf16* __restrict__ C, int ldc, const __bf16* __restrict__ G,
                                                       const __bf16* __restrict__ R, int M, int N, int K, int tiles_m, int tiles_n, int remap) {
    __shared__ __attribute__((aligned(1024))) char smem[2 * P8_BUF];
    const int wg = remap ? xcd_remap(blockIdx.x, tiles_m * tiles_n) : (int)blockIdx.x;
    const int tm = wg / tiles_n, tn = wg - tm * tiles_n;
    const int m0 = tm * 256, n0 = tn * 256;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wr = wave >> 2, wc = wave & 3;

    P8tPolicy pol{{}, {}, (size_t)P8_BK * ldb, frag_off(lane), FragTr(lane)};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        pol.ga[h] = p8_krow_src(A, lda, m0 + 128 * h, M, wave, lane);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int kr = 8 * wave + 4 * u + (lane >> 4);
            const int col = min(n0 + 128 * h + 8 * ((lane & 15) ^ tr_swizzle(kr)), N - 8);      // columns past N are clamped (their sums are never stored)
            pol.gb[h][u] = B + (size_t)kr * ldb + col;
        }
    }
    floatx4 acc[8][4];
    p8_main_loop(pol, acc, smem, K / P8_BK, wave);

    char* wl = smem + wave * 16384;                      // 16 KiB of the free ring per wave
    const int row0 = m0 + wr * 128, col0 = n0 + wc * 64;
    p8t_store_half<GACT, HASR>(acc, 0, C, G, R, ldc, row0, col0, M, N, lane, wl);
    p8t_store_half<GACT, HASR>(acc, 1, C, G, R, ldc, row0, col0, M, N, lane, wl);
}

extern "C" {

// 1 if this (shape, layout) runs on the p8t kernel: A bf16 [M][lda] k-contiguous, B bf16 [K][ldb] (k-strided), C / G / R bf16 [M][ldc]
int svpc_gemm_p8t_supported(int lda, int ldb, int ldc, int M, int N, int K) {
    return (M > 0 && N >= 8 && (N & 7) == 0 && K >= P8_BK && K % P8_BK == 0 && (lda & 7) == 0 && (ldb & 7) == 0 && (ldc & 7) == 0 && lda >= K &&
            ldb >= N && ldc >= N) ? 1 : 0;
}

// C = (A·B) ⊙ gact'(G) + R.  gact: SVPC_ACT_NONE / RELU / GELU (G = the pre-activation or activated tensor the forward kept; the
// derivative as svpc_act_bwd, GELU by the A&S erf of svpc_gemm_glds_rg's epilogue); G, R optional (NULL).
int svpc_gemm_p8t(const void* A, int lda, const void* B, int ldb, void* C, int ldc, const void* G, int gact, const void* R, int M, int N, int K,
                  hipStream_t stream) {
    if (M <= 0 || N <= 0) return 0;
    if (G == nullptr) gact = ACT_NONE;
    SVPC_REQUIRE(svpc_gemm_p8t_supported(lda, ldb, ldc, M, N, K) == 1 &&
                     ((((uintptr_t)A) | ((uintptr_t)B) | ((uintptr_t)C) | ((uintptr_t)G) | ((uintptr_t)R)) & 15) == 0 &&
                     (gact == ACT_NONE || gact == ACT_RELU || gact == ACT_GELU),
                 "gemm_p8t: needs K % 64 == 0, N % 8 == 0, 16-byte aligned bf16 rows, gact in {none, relu, gelu}");
    const int remap = gemm_remap_env();
    const int tiles_m = ceil_div(M, 256), tiles_n = ceil_div(N, 256);
#define P8T_GO(GA, HR)                                                                                                           \
    hipLaunchKernelGGL((gemm_p8t_kernel<GA, HR>), dim3(tiles_m * tiles_n), dim3(512), 0, stream, (const __bf16*)A, lda, (const __bf16*)B, \
                       ldb, (__bf16*)C, ldc, (const __bf16*)G, (const __bf16*)R, M, N, K, tiles_m, tiles_n, remap)
    const bool hr = R != nullptr;
    if (gact == ACT_GELU) { if (hr) P8T_GO(ACT_GELU, true); else P8T_GO(ACT_GELU, false); }
    else if (gact == ACT_RELU) { if (hr) P8T_GO(ACT_RELU, true); else P8T_GO(ACT_RELU, false); }
    else { if (hr) P8T_GO(ACT_NONE, true); else P8T_GO(ACT_NONE, false); }
#undef P8T_GO
    return svpc_check_launch("gemm_p8t");
}

}  // extern "C"
