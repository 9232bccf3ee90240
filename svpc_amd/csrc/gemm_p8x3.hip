// Three-term split-bf16 GEMM ("bf16x3") for the forward projections of the activation streams in the ≤1e-4-parity throughput mode:
//
//   C = act( A·Bᵀ + bias ),  A = A_hi + A_lo,  B = B_hi + B_lo  (each an exact sum of two bf16 planes, 16-17 significant bits)
//   A·Bᵀ ≈ A_lo·B_hiᵀ + A_hi·B_hiᵀ + A_hi·B_loᵀ          (the dropped A_lo·B_lo term is ≤ 2⁻¹⁶ relative)
//
// The 256×256 8-phase main loop of gemm_common.h with ONE difference in what a staged buffer holds: the two 32-wide "k blocks" of a
// half-tile image are the HI and the LO plane of the same 32-deep k-slice (not two consecutive k blocks of one plane).  A buffer then
// carries everything the three products of its slice need — A_hi, A_lo, B_hi, B_lo fetched ONCE, their
// fragments read from LDS ONCE — and every phase issues 24 MFMAs (lo·hi, hi·hi, hi·lo per output block) on the 12 fragments that fed 16:
// the kernel is bound by the LDS fill rate of a CU (≈40–50 GB/s direct-to-LDS from L2 / Infinity Cache: MI355X_MICROARCH.md "gather
// into LDS"), so 1.5× the matrix work per staged byte is what pays (round 3, first form: a 3K-deep contraction of three plane pairs,
// every hi tile staged twice — 6 tiles per 64-deep slice instead of 4).  fp32 accumulation of bf16 products is exact per product, so the
// result carries ≈ fp32 accuracy at 3× the bf16 MFMA work — against 16× for the f32 MFMA (MI355X_MICROARCH.md: f32-input MFMA runs at
// 1/16 of the bf16 rate).
//
// Storage ("split16", see layernorm.hip): a row of A holds its hi plane at columns [0, K) and its lo plane at [a_lo, a_lo + K); the
// weight shadow keeps two planes of identical layout b_lo elements apart; C is written the same way (hi at column c, lo at c_lo + c).
// The hi plane alone is the RNE-rounded bf16 tensor the bf16 backward kernels (dgrad / wgrad / LayerNorm / attention) read in place.
// The optional pre-activation copy Z (what the GELU backward differentiates) is a plain bf16 matrix.
//
// reference ops replaced: every nn.Linear forward of the clip encoder (src/rtransformer/model.py:195-197, :230, :259, :281, :551).
#include "gemm_common.h"

constexpr int X3_KS = 32;            // k-slice per staged buffer

struct X3Policy {
    static constexpr int MIN_NK = 2;      // K ≥ 64: there always is a slice 1
    static constexpr bool THREE_TERM = true;
    const __bf16* ga[2];
    const __bf16* gb[2];
    int a_lo;
    long long b_lo;
    int fr_off;
    // buffer t = k-slice t (32 deep): "k block" 0 of every half-tile image is the slice of the hi plane, "k block" 1 the slice of the
    // lo plane (element offsets from the hi-plane row pointers)
    template <int W>
    __device__ __forceinline__ void stage(int t, char* dst) const {
        const __bf16* src = (W < 2 ? ga[W & 1] : gb[W & 1]) + (size_t)t * X3_KS;
        p8_dma2(src, src + (W < 2 ? (size_t)a_lo : (size_t)b_lo), dst);
    }
    __device__ __forceinline__ bf16x8 frag_a(const char* img, int blk, int kb) const { return frag_rd(img, blk, kb, fr_off); }
    __device__ __forceinline__ bf16x8 frag_b(const char* img, int cb, int kb) const { return frag_rd(img, cb, kb, fr_off); }
    template <int PH>
    __device__ __forceinline__ void extra(const bf16x8 (&)[2][4]) const {}
};

template <int ACT, bool HASZ>
__global__ __launch_bounds__(512) void gemm_p8x3_kernel(const __bf16* __restrict__ A, int lda, int a_lo, const __bf16* __restrict__ B, int ldb,
                                                        long long b_lo, __bf16* __restrict__ C, int ldc, int c_lo, __bf16* __restrict__ Z,
                                                        int ldz, const float* __restrict__ bias, int M, int N, int K, int tiles_m,
                                                        int tiles_n, int remap) {
    __shared__ __attribute__((aligned(1024))) char smem[2 * P8_BUF];
    const int wg = remap ? xcd_remap(blockIdx.x, tiles_m * tiles_n) : (int)blockIdx.x;
    const int tm = wg / tiles_n, tn = wg - tm * tiles_n;
    const int m0 = tm * 256, n0 = tn * 256;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wr = wave >> 2, wc = wave & 3;

    X3Policy pol{{}, {}, a_lo, b_lo, frag_off(lane)};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        pol.ga[h] = p8_krow_src(A, lda, m0 + 128 * h, M, wave, lane);
        pol.gb[h] = p8_krow_src(B, ldb, n0 + 128 * h, N, wave, lane);
    }
    floatx4 acc[8][4];
    p8_main_loop(pol, acc, smem, K / X3_KS, wave);       // staged buffers = 32-deep k-slices (hi and lo plane of both operands)

    char* wl = smem + wave * 16384;                      // 16 KiB of the free ring per wave
    const int row0 = m0 + wr * 128, col0 = n0 + wc * 64;
    float4 bb[4];
    p8_load_bias(bb, bias, col0, N, lane);
    if (HASZ) p8_store_pass<ACT, SV_PRE>(acc, Z, ldz, bb, row0, col0, M, N, lane, wl);
    p8_store_pass<ACT, SV_LO>(acc, C + c_lo, ldc, bb, row0, col0, M, N, lane, wl);
    p8_store_pass<ACT, SV_HI>(acc, C, ldc, bb, row0, col0, M, N, lane, wl);
}

extern "C" {

// 1 if (shape, layout) runs on this kernel
int svpc_gemm_p8x3_supported(int lda, int a_lo, int ldb, int ldc, int c_lo, int ldz, int M, int N, int K) {
    if (M <= 0 || N <= 0 || K < 2 * X3_KS || K % X3_KS != 0 || (N & 7) != 0) return 0;
    if ((lda & 7) || (a_lo & 7) || (ldb & 7) || (ldc & 7) || (c_lo & 7) || (ldz & 7)) return 0;
    if (a_lo < K || lda < a_lo + K || c_lo < N || ldc < c_lo + N || ldb < K) return 0;
    if ((unsigned long long)M * (unsigned long long)ldc * 2ull >= (1ull << 32)) return 0;
    if ((unsigned long long)M * (unsigned long long)(ldz > 0 ? ldz : 1) * 2ull >= (1ull << 32)) return 0;
    return 1;
}

// C (split) = act(A (split) · B (split)ᵀ + bias); A [M][lda] with planes at columns 0 / a_lo; B_hi [N][ldb] and B_lo = B_hi + b_lo
// elements (same layout); C [M][ldc] planes at columns 0 / c_lo; Z (optional, only with an activation): plain bf16 [M][ldz]
// pre-activation (without an activation it would equal C's hi plane).
int svpc_gemm_p8x3(const void* A, int lda, int a_lo, const void* B, int ldb, long long b_lo, void* C, int ldc, int c_lo, void* Z, int ldz,
                   int M, int N, int K, const float* bias, int act, hipStream_t stream) {
    if (M <= 0 || N <= 0) return 0;
    if (Z == nullptr) ldz = 0;
    SVPC_REQUIRE(svpc_gemm_p8x3_supported(lda, a_lo, ldb, ldc, c_lo, ldz, M, N, K) == 1 && (b_lo & 7) == 0 &&
                     ((((uintptr_t)A) | ((uintptr_t)B) | ((uintptr_t)C) | ((uintptr_t)Z) | ((uintptr_t)bias)) & 15) == 0 &&
                     (act == ACT_RELU || act == ACT_GELU || (act == ACT_NONE && Z == nullptr)) && (Z == nullptr || ldz >= N),
                 "gemm_p8x3: needs K % 32 == 0, K >= 64, N % 8 == 0, 16-byte aligned split rows (lo plane behind the hi plane), act in {none, relu, gelu}");
    const int remap = gemm_remap_env();
    const int tiles_m = ceil_div(M, 256), tiles_n = ceil_div(N, 256);
#define X3_GO(ACTV, ZV)                                                                                                          \
    hipLaunchKernelGGL((gemm_p8x3_kernel<ACTV, ZV>), dim3(tiles_m * tiles_n), dim3(512), 0, stream, (const __bf16*)A, lda, a_lo,  \
                       (const __bf16*)B, ldb, b_lo, (__bf16*)C, ldc, c_lo, (__bf16*)Z, ldz, bias, M, N, K, tiles_m, tiles_n, remap)
    const bool z = Z != nullptr;
    if (act == ACT_GELU) { if (z) X3_GO(ACT_GELU, true); else X3_GO(ACT_GELU, false); }
    else if (act == ACT_RELU) { if (z) X3_GO(ACT_RELU, true); else X3_GO(ACT_RELU, false); }
    else X3_GO(ACT_NONE, false);
#undef X3_GO
    return svpc_check_launch("gemm_p8x3");
}

}  // extern "C"
