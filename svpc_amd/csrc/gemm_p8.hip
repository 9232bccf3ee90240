// bf16 × bf16 → bf16 GEMM for the forward projections of the bf16 activation streams ("p8"): the 256×256 8-phase main loop of
// gemm_common.h with both operands k-contiguous (st_16x32 images, plain ds_read_b128 fragments).
//
//   C[M,N] = act( A[M,K]·B[N,K]ᵀ + bias )  (+ optional pre-activation copy Z),  K % 64 == 0, any M, N % 8 == 0
//
// Epilogue: a lane's 4 consecutive columns of an output row are packed to bf16 and pass through a wave-private LDS image so that every
// global store instruction writes whole 128-byte lines (p8_store_pass; the ring is free by then).
#include "gemm_common.h"

struct P8Policy {
    static constexpr int MIN_NK = 1;
    static constexpr bool THREE_TERM = false;
    const __bf16* ga[2];
    const __bf16* gb[2];
    int fr_off;
    template <int W>
    __device__ __forceinline__ void stage(int t, char* dst) const {
        const __bf16* src = (W < 2 ? ga[W & 1] : gb[W & 1]) + (size_t)t * P8_BK;
        p8_dma2(src, src + 32, dst);
    }
    __device__ __forceinline__ bf16x8 frag_a(const char* img, int blk, int kb) const { return frag_rd(img, blk, kb, fr_off); }
    __device__ __forceinline__ bf16x8 frag_b(const char* img, int cb, int kb) const { return frag_rd(img, cb, kb, fr_off); }
    template <int PH>
    __device__ __forceinline__ void extra(const bf16x8 (&)[2][4]) const {}
};

template <int ACT, bool HASZ>
__global__ __launch_bounds__(512) void gemm_p8_kernel(const __bf16* __restrict__ A, int lda, const __bf16* __restrict__ B, int ldb,
                                                      __bf16* __restrict__ C, int ldc, int M, int N, int K, Epi epi, int tiles_m,
                                                      int tiles_n, int remap) {
    __shared__ __attribute__((aligned(1024))) char smem[2 * P8_BUF];
    const int wg = remap ? xcd_remap(blockIdx.x, tiles_m * tiles_n) : (int)blockIdx.x;
    const int tm = wg / tiles_n, tn = wg - tm * tiles_n;
    const int m0 = tm * 256, n0 = tn * 256;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wr = wave >> 2, wc = wave & 3;

    P8Policy pol;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        pol.ga[h] = p8_krow_src(A, lda, m0 + 128 * h, M, wave, lane);
        pol.gb[h] = p8_krow_src(B, ldb, n0 + 128 * h, N, wave, lane);
    }
    pol.fr_off = frag_off(lane);
    floatx4 acc[8][4];
    p8_main_loop(pol, acc, smem, K / P8_BK, wave);

    char* wl = smem + wave * 16384;                      // 16 KiB of the free ring per wave
    const int row0 = m0 + wr * 128, col0 = n0 + wc * 64;
    float4 bb[4];
    p8_load_bias(bb, epi.bias, col0, N, lane);
    // pre-activation copy first: the activation pass then consumes the sums for the last time and its registers free up as it goes
    if (HASZ) p8_store_pass<ACT, SV_PRE>(acc, reinterpret_cast<__bf16*>(epi.Z), ldc, bb, row0, col0, M, N, lane, wl);
    p8_store_pass<ACT, SV_ACT>(acc, C, ldc, bb, row0, col0, M, N, lane, wl);
}

// 1 if this (shape, epilogue) runs on the p8 kernel; the launcher of gemm_glds.hip asks before choosing its own 256×256 form
bool glds_p8_supported(int a_kc, int b_kc, int c_dt, int lda, int ldb, int ldc, int M, int N, int K, const Epi& epi, const void* A,
                       const void* B, const void* C) {
    return a_kc && b_kc && c_dt == 1 && K >= P8_BK && K % P8_BK == 0 && (N & 7) == 0 && (ldc & 7) == 0 && (lda & 7) == 0 &&
           (ldb & 7) == 0 && epi.p_drop <= 0.f && !epi.accumulate && epi.R == nullptr && epi.G == nullptr && epi.act != ACT_SIGMOID &&
           (unsigned long long)M * (unsigned long long)ldc * 2ull < (1ull << 32) &&
           ((((uintptr_t)A) | ((uintptr_t)B) | ((uintptr_t)C) | ((uintptr_t)epi.Z) | ((uintptr_t)epi.bias)) & 15) == 0;
}
int glds_p8_launch(const void* A, int lda, const void* B, int ldb, void* C, int ldc, int M, int N, int K, const Epi& epi, int remap,
                   hipStream_t stream) {
    const int tiles_m = ceil_div(M, 256), tiles_n = ceil_div(N, 256);
    // one instantiation per (activation, pre-activation copy): each epilogue is register-allocated on its own
#define P8_GO(ACTV, ZV)                                                                                                         \
    hipLaunchKernelGGL((gemm_p8_kernel<ACTV, ZV>), dim3(tiles_m * tiles_n), dim3(512), 0, stream, (const __bf16*)A, lda, (const __bf16*)B, \
                       ldb, (__bf16*)C, ldc, M, N, K, epi, tiles_m, tiles_n, remap)
    const bool z = epi.Z != nullptr;
    if (epi.act == ACT_GELU) { if (z) P8_GO(ACT_GELU, true); else P8_GO(ACT_GELU, false); }
    else if (epi.act == ACT_RELU) { if (z) P8_GO(ACT_RELU, true); else P8_GO(ACT_RELU, false); }
    else { if (z) P8_GO(ACT_NONE, true); else P8_GO(ACT_NONE, false); }
#undef P8_GO
    return svpc_check_launch("gemm_p8");
}

extern "C" int svpc_gemm_p8(const void* A, int lda, const void* B, int ldb, void* C, int ldc, void* Z, int M, int N, int K, const float* bias,
                            int act, hipStream_t stream) {
    if (M <= 0 || N <= 0) return 0;
    Epi epi{bias, act, 0.f, 0u, nullptr, 0, (float*)Z, nullptr};
    SVPC_REQUIRE(glds_p8_supported(1, 1, 1, lda, ldb, ldc, M, N, K, epi, A, B, C),
                 "gemm_p8: needs K % 64 == 0, N % 8 == 0, 16-byte aligned bf16 rows, act in {none, relu, gelu}");
    return glds_p8_launch(A, lda, B, ldb, C, ldc, M, N, K, epi, gemm_remap_env(), stream);
}
