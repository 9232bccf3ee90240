// Shared by the GEMM families: the element-wise epilogue (bias, activation, dropout, pre-activation store, accumulate), the XCD remap
// and its cached switch, the split-K reducer, the small value helpers of the bf16 kernels (A&S-erf GELU, pack2, split residual, the two
// swizzled LDS fragment reads), and — in a section of its own at the end — the ONE 8-phase main loop of the 256×256 kernels
// (gemm_p8.hip, gemm_p8t.hip, gemm_p8w.hip, gemm_p8x3.hip) with their whole-line store pass.
#pragma once
#include "common.h"
#include <stdlib.h>

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef const void __attribute__((address_space(1))) * gemm_gptr;      // the two pointer kinds of __builtin_amdgcn_global_load_lds
typedef void __attribute__((address_space(3))) * gemm_lptr;

struct Epi {
    const float* bias; int act; float p_drop; uint32_t site; const u64* seed; int accumulate;
    float* Z;   // optional pre-activation output (same ldc)
    const void* R;   // optional addend of C's type and layout, C = act(acc + bias) + R (a residual-path gradient joining a dgrad).  bf16: only
                     // the 16-byte row-store epilogues of gemm_glds.hip apply it (the launcher refuses R where they cannot run);
                     // fp32: the element-wise epilogues below (svpc_gemm_l32_r)
    const void* G; int gact;   // optional: C = (A·B) ⊙ gact'(G) (+ R) — G of C's type and layout is what the forward of activation `gact` kept
                               // (z for GELU, y for ReLU / sigmoid): a dgrad whose output feeds an activation's backward applies it.
                               // bf16: like a bf16 R only in the 16-byte row-store epilogues of gemm_glds.hip (the launcher refuses it
                               // elsewhere); fp32: the element-wise epilogue below (svpc_gemm_l32_rg)
};

__device__ __forceinline__ void epilogue_store(float v, int row, int col, float* __restrict__ C, int ldc, const Epi& e,
                                               u64 seed, float inv_keep) {
    if (e.bias) v += e.bias[col];
    const size_t o = (size_t)row * ldc + col;
    if (e.Z) e.Z[o] = v;
    v = apply_act(v, e.act);
    if (e.p_drop > 0.f) v *= drop_scale(seed, e.site, o, e.p_drop, inv_keep);
    if (e.G) v *= act_grad_from_aux(reinterpret_cast<const float*>(e.G)[o], e.gact, false);      // (fp32 G: svpc_gemm_l32_rg)
    if (e.accumulate) v += C[o];
    if (e.R) v += reinterpret_cast<const float*>(e.R)[o];
    C[o] = v;
}


// The same epilogue for NE elements of one thread at once: every load it needs (bias, the old C of an accumulate, R, G) is issued before
// the first is consumed.  Called element by element (epilogue_store in a loop) each conditional load sits in a region of its own and the
// compiler drains the memory counter behind every one of them — NE × (features) dependent round trips per thread.  `row` / `col` must be
// valid (clamped) coordinates for every element; `ok[k]` says whether element k is stored.  Same arithmetic, same order.
template <int NE>
__device__ __forceinline__ void epilogue_store_n(const float (&vin)[NE], const int (&row)[NE], const int (&col)[NE], const bool (&ok)[NE],
                                                 float* __restrict__ C, int ldc, const Epi& e, u64 seed, float inv_keep) {
    size_t o[NE];
    float b[NE], old[NE], r[NE], g[NE];
#pragma unroll
    for (int k = 0; k < NE; ++k) { o[k] = (size_t)row[k] * ldc + col[k]; b[k] = 0.f; old[k] = 0.f; r[k] = 0.f; g[k] = 0.f; }
    if (e.bias) {
#pragma unroll
        for (int k = 0; k < NE; ++k) b[k] = e.bias[col[k]];
    }
    if (e.accumulate) {
#pragma unroll
        for (int k = 0; k < NE; ++k) old[k] = C[o[k]];
    }
    if (e.R) {
#pragma unroll
        for (int k = 0; k < NE; ++k) r[k] = reinterpret_cast<const float*>(e.R)[o[k]];
    }
    if (e.G) {
#pragma unroll
        for (int k = 0; k < NE; ++k) g[k] = reinterpret_cast<const float*>(e.G)[o[k]];
    }
    float v[NE];
#pragma unroll
    for (int k = 0; k < NE; ++k) v[k] = vin[k] + b[k];
    if (e.Z) {
#pragma unroll
        for (int k = 0; k < NE; ++k)
            if (ok[k]) e.Z[o[k]] = v[k];
    }
#pragma unroll
    for (int k = 0; k < NE; ++k) {
        float t = apply_act(v[k], e.act);
        if (e.p_drop > 0.f) t *= drop_scale(seed, e.site, o[k], e.p_drop, inv_keep);
        if (e.G) t *= act_grad_from_aux(g[k], e.gact, false);
        v[k] = (t + old[k]) + r[k];
    }
    bool all_ok = true;
#pragma unroll
    for (int k = 0; k < NE; ++k) all_ok = all_ok && ok[k];
    if (__all(all_ok)) {                                  // interior (wave-uniform): stores back to back, no exec-masked regions
#pragma unroll
        for (int k = 0; k < NE; ++k) C[o[k]] = v[k];
    } else {
#pragma unroll
        for (int k = 0; k < NE; ++k)
            if (ok[k]) C[o[k]] = v[k];
    }
}

// typed variant: C and the optional pre-activation copy Z are stored as TC (float or __bf16)
template <typename TC>
__device__ __forceinline__ void epilogue_store_t(float v, int row, int col, TC* __restrict__ C, int ldc, const Epi& e, u64 seed,
                                                 float inv_keep) {
    if (e.bias) v += e.bias[col];
    const size_t o = (size_t)row * ldc + col;
    if (e.Z) reinterpret_cast<TC*>(e.Z)[o] = (TC)v;
    v = apply_act(v, e.act);
    if (e.p_drop > 0.f) v *= drop_scale(seed, e.site, o, e.p_drop, inv_keep);
    if (e.accumulate) v += (float)C[o];
    if (sizeof(TC) == 4 && e.R) v += reinterpret_cast<const float*>(e.R)[o];      // (bf16 addends: gemm_glds.hip's row-store epilogues)
    C[o] = (TC)v;
}

// XCD-aware bijective remap of a linear workgroup id: ids that share an XCD (id % 8) get a contiguous tile range,
// so tiles sharing an operand panel hit the same private L2.
__device__ __forceinline__ int xcd_remap(int orig, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, xcd = orig & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (orig >> 3);
}
// SVPC_GEMM_REMAP (default 1): 0 turns the remap off in every tiled launcher; read once
static inline int gemm_remap_env() {
    static int remap = -1;
    if (remap < 0) { const char* e = getenv("SVPC_GEMM_REMAP"); remap = e ? atoi(e) : 1; }
    return remap;
}


// ---- split-K tail shared by the MFMA GEMM families: C = epi( Σ_k slabs[k] ), slabs summed in k order (deterministic).
// The vector form handles 4 consecutive columns per thread with 4 slab loads in flight (N % 4 == 0); the sum order per
// element is the same as in the scalar form, so both give identical bits.
template <typename TC>
__global__ __launch_bounds__(256) void splitk_reduce1_kernel(const float* __restrict__ slabs, int splitk, TC* __restrict__ C, int ldc,
                                                             int M, int N, Epi epi) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)M * N) return;
    const int row = (int)(i / N), col = (int)(i - (size_t)row * N);
    float s = 0.f;
    for (int k = 0; k < splitk; ++k) s += slabs[(size_t)k * M * N + i];
    const u64 seed = epi.p_drop > 0.f ? epi.seed[0] : 0ull;
    const float inv_keep = epi.p_drop > 0.f ? 1.0f / (1.0f - epi.p_drop) : 1.0f;
    epilogue_store_t<TC>(s, row, col, C, ldc, epi, seed, inv_keep);
}
template <typename TC>
__global__ __launch_bounds__(256) void splitk_reduce4_kernel(const float* __restrict__ slabs, int splitk, TC* __restrict__ C, int ldc,
                                                             int M, int N, Epi epi) {
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x, nq = (size_t)M * N / 4;
    if (q >= nq) return;
    const size_t i = q * 4;
    const int row = (int)(i / N), col = (int)(i - (size_t)row * N);
    const float4* p = reinterpret_cast<const float4*>(slabs) + q;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    int k = 0;
    for (; k + 4 <= splitk; k += 4) {
        const float4 a = p[(size_t)k * nq], b = p[(size_t)(k + 1) * nq], c = p[(size_t)(k + 2) * nq], d = p[(size_t)(k + 3) * nq];
        s.x += a.x; s.y += a.y; s.z += a.z; s.w += a.w;
        s.x += b.x; s.y += b.y; s.z += b.z; s.w += b.w;
        s.x += c.x; s.y += c.y; s.z += c.z; s.w += c.w;
        s.x += d.x; s.y += d.y; s.z += d.z; s.w += d.w;
    }
    for (; k < splitk; ++k) {
        const float4 a = p[(size_t)k * nq];
        s.x += a.x; s.y += a.y; s.z += a.z; s.w += a.w;
    }
    const u64 seed = epi.p_drop > 0.f ? epi.seed[0] : 0ull;
    const float inv_keep = epi.p_drop > 0.f ? 1.0f / (1.0f - epi.p_drop) : 1.0f;
    epilogue_store_t<TC>(s.x, row, col, C, ldc, epi, seed, inv_keep);
    epilogue_store_t<TC>(s.y, row, col + 1, C, ldc, epi, seed, inv_keep);
    epilogue_store_t<TC>(s.z, row, col + 2, C, ldc, epi, seed, inv_keep);
    epilogue_store_t<TC>(s.w, row, col + 3, C, ldc, epi, seed, inv_keep);
}
template <typename TC>
static inline void launch_splitk_reduce(const float* slabs, int splitk, TC* C, int ldc, int M, int N, const Epi& epi, hipStream_t stream) {
    const size_t n = (size_t)M * N;
    if (N % 4 == 0 && ((((uintptr_t)slabs) & 15) == 0))
        hipLaunchKernelGGL(splitk_reduce4_kernel<TC>, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, stream, slabs, splitk, C, ldc, M, N,
                           epi);
    else
        hipLaunchKernelGGL(splitk_reduce1_kernel<TC>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, slabs, splitk, C, ldc, M, N, epi);
}


// ---- value helpers of the bf16 MFMA kernels (gemm_p8*.hip, gemm_s4*.hip)
__device__ __forceinline__ uint32_t pack2(float lo, float hi) {
    union { __bf16 h[2]; uint32_t u; } pk;
    pk.h[0] = (__bf16)lo; pk.h[1] = (__bf16)hi;
    return pk.u;
}
// residual of the bf16 rounding, itself rounded to bf16 when stored: v ≈ hi + lo to 2⁻¹⁷ (the lo plane of a split tensor)
__device__ __forceinline__ float bf16_lo(float v) { return v - (float)(__bf16)v; }

// GELU with erf by Abramowitz-Stegun 7.1.26 (|error| <= 1.5e-7 + the 1-ulp rcp/exp: three orders below the 2^-9 rounding of a bf16
// value, and below the 2⁻¹⁷ of a stored hi/lo pair), branch-free, ~14 instructions per element instead of the ~60 of the exact library
// routine — the tail of a 256x256 tile evaluates it 65,536 times per workgroup with nothing left to overlap it.  The pre-activation copy
// Z (what the backward differentiates) is the exact sum; the fp32 parity mode never comes here (gemm.hip, exact erff).
__device__ __forceinline__ float gelu_as(float x) {
    const float u = x * 0.70710678118654752f, au = fabsf(u);
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, au, 1.0f));
    float p = fmaf(1.061405429f, t, -1.453152027f);
    p = fmaf(p, t, 1.421413741f);
    p = fmaf(p, t, -0.284496736f);
    p = fmaf(p, t, 0.254829592f);
    const float e = __expf(-au * au);
    const float erf_abs = fmaf(-p * t, e, 1.0f);
    return 0.5f * x * (1.0f + copysignf(erf_abs, u));
}
template <int ACT>
__device__ __forceinline__ float gemm_act(float z) {
    if (ACT == ACT_RELU) return fmaxf(z, 0.f);
    if (ACT == ACT_GELU) return gelu_as(z);
    return z;
}

// ---- the two LDS tile images and their MFMA fragment reads (v_mfma_f32_16x16x32_bf16: a lane holds 8 consecutive k of one row / column).
// st_16x32 (k-contiguous operand rows): an image is 1-KiB subtiles of [16 rows][32 k] bf16, subtile (row block blk, k block kb) at
// ((blk·2 + kb) << 10); the 16-byte chunk c of rows 8-15 is kept at c ^ 2, applied on the per-lane SOURCE address of the LDS-DMA and on
// the read address (never on the LDS destination): ds_read_b128 without bank conflicts.  Lane: row lane&15, logical chunk lane>>4.
__device__ __forceinline__ int frag_off(int lane) { return (lane & 15) * 64 + ((((lane >> 4) ^ (((lane >> 3) & 1) << 1))) << 4); }
__device__ __forceinline__ bf16x8 frag_rd(const char* img, int blk, int kb, int fr_off) {
    return *reinterpret_cast<const bf16x8*>(img + ((blk * 2 + kb) << 10) + fr_off);
}
// k-strided operand (rows as they lie in memory): an image is [64 k-rows][128 columns], 1 KiB = 4 k-rows per DMA wave-instruction, read
// with ds_read_b64_tr_b16: within a group of 16 lanes the instruction reads a 4-row × 16-column block and hands lane li the four rows of
// column li — two of them give a lane the 8 consecutive k of its column.  Bank conflicts: rows are 256 bytes (= all 64 banks), so the
// 16-byte chunk c of k-row r is kept at slot c ^ tr_swizzle(r) — the eight rows a half-wave touches land in eight disjoint 8-bank
// windows (again applied on the DMA source address and on the read address).
__device__ __forceinline__ int tr_swizzle(int kr) { return 2 * ((kr & 3) | ((kr >> 1) & 4)); }
struct FragTr {
    int off, fx, p1;
    // lane (g = lane>>4, q = (lane&15)>>2, p = lane&3) reads k-rows 32·kb + 8g + q (+4) at logical chunk 2·cb + (p>>1), byte (p&1)·8;
    // both rows share the swizzle 2·(q + 4·(g&1))
    __device__ __forceinline__ explicit FragTr(int lane) {
        const int tg = lane >> 4, tq = (lane & 15) >> 2, tp = lane & 3;
        fx = 2 * (tq + 4 * (tg & 1));
        off = (8 * tg + tq) * 256 + ((tp & 1) << 3);
        p1 = tp >> 1;
    }
    // 16-column block cb (0..7) and k block kb of the image.  (__restrict__ stays: without it the compiler puts a full vmcnt(0) drain in
    // front of the first read of every k-tile of gemm_s4t.hip — no LDS-DMA left in flight — and the training step measured 1.5 % slower.)
    __device__ __forceinline__ bf16x8 operator()(const char* __restrict__ img, int cb, int kb) const {
        typedef short short4v __attribute__((ext_vector_type(4)));
        typedef short4v __attribute__((address_space(3))) * lds_ptr;
        const char* a = img + kb * (32 * 256) + off + (((((2 * cb) ^ fx)) | p1) << 4);
        const short4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(a));                  // rows r..r+3 of the lane's column
        const short4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(a + 4 * 256));        // rows r+4..r+7
        union { short s[8]; bf16x8 v; } u;
        u.s[0] = lo[0]; u.s[1] = lo[1]; u.s[2] = lo[2]; u.s[3] = lo[3];
        u.s[4] = hi[0]; u.s[5] = hi[1]; u.s[6] = hi[2]; u.s[7] = hi[3];
        return u.v;
    }
};


// =====================================================================================================================================
// The 256×256 8-phase family: ONE main loop for gemm_p8.hip, gemm_p8t.hip, gemm_p8w.hip and gemm_p8x3.hip
// (cdna_hip_programming.md §5 "The 256² 8-phase template", rebuilt for this library's operand layouts).
//   * 8 waves = two groups (waves 0-3 / 4-7, one of each per SIMD) running ONE barrier interval apart: while a group issues the MFMAs
//     of a phase (a 64×32 quadrant of its 128×64 wave tile over one k-tile), the other reads the fragments of its next phase from LDS
//     and issues its share of the LDS-DMA prefetch — a SIMD's matrix pipe always has exactly one wave feeding it.
//   * LDS: two 64-KiB buffers, each four staged half-tiles (A rows 0-127 / 128-255, B columns 0-127 / 128-255 of one k-tile) in one of
//     the two images above; every wave issues two 1-KiB DMA wave-instructions per half-tile, to the destination the loop hands it.
//   * Prefetch: phase p of k-tile t stages half-tile p of what comes next — A halves of tile t+1 in phases 0,1 (their buffer's last
//     A read was phase 2 of tile t-1), B halves of tile t+2 in phases 2,3 (this buffer's last B read was phase 1 of tile t; the
//     first B fragments, needed again in phase 3, stay in registers).  ONE counted wait per k-tile (vmcnt(4): the two B halves of tile
//     t+2 stay in flight), placed one barrier before the first read of tile t+1 by either group; raw s_barrier only.
//   * Operands swapped in the MFMA (the B operand in the instruction's A slot): a lane holds 4 consecutive columns of ONE output row.
// A kernel supplies a policy P:
//   P::MIN_NK                 the least number of k-tiles the launcher lets through (2: the prologue stages tile 1 unasked; 0: none)
//   P::THREE_TERM             false: the two k blocks of an image are consecutive k, 16 MFMAs per phase;
//                             true:  they are the hi and the lo plane of one k-slice, 24 MFMAs per phase (lo·hi, hi·hi, hi·lo)
//   stage<W>(t, dst)          the two LDS-DMA instructions of half-tile W (0 A0, 1 A1, 2 B0, 3 B1) of k-tile t → dst, dst + 1024
//   frag_a(img, blk, kb)      the A fragment of 16-row block blk, k block kb of a half-tile image;  frag_b(img, cb, kb) likewise for B
//   extra<PH>(afr)            more MFMAs on the A fragments of phase PH (0 or 2) while they are in registers
constexpr int P8_BK = 64;
constexpr int P8_HALF = 128 * P8_BK * 2;      // 16 KiB: one staged half-tile
constexpr int P8_BUF = 4 * P8_HALF;           // 64 KiB: A0 A1 B0 B1 of one k-tile

__device__ __forceinline__ void p8_sync() {
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
}
// every DMA of k-tile t+1 issued by this wave has landed (the two B halves of tile t+2, issued after them, may stay in flight)
__device__ __forceinline__ void p8_wait(int t, int nk) {
    if (t + 2 < nk) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
template <int W, class P>
__device__ __forceinline__ void p8_stage(P& pol, char* my, int t) { pol.template stage<W>(t, my + (t & 1) * P8_BUF + W * P8_HALF); }
// the MFMAs of one phase: the 4×2 blocks at (I0, J0) of the wave tile
template <bool THREE_TERM, int I0, int J0>
__device__ __forceinline__ void p8_mma(floatx4 (&acc)[8][4], const bf16x8 (&b)[2][2], const bf16x8 (&a)[2][4]) {
    if (THREE_TERM) {
#pragma unroll
        for (int term = 0; term < 3; ++term)            // lo·hi, hi·hi, hi·lo: plane 1 = lo
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[I0 + i][J0 + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[term == 2 ? 1 : 0][j], a[term == 0 ? 1 : 0][i], acc[I0 + i][J0 + j], 0, 0, 0);
    } else {
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[I0 + i][J0 + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[kb][j], a[kb][i], acc[I0 + i][J0 + j], 0, 0, 0);
    }
}

// acc = Σ over nk k-tiles; smem: the two buffers (128 KiB, 1-KiB aligned); wave = threadIdx.x >> 6, wave-uniform.  On return every wave
// is past its last LDS read and every LDS-DMA has landed: the ring is free.
template <class P>
__device__ __forceinline__ void p8_main_loop(P& pol, floatx4 (&acc)[8][4], char* __restrict__ smem, int nk, int wave) {
    __builtin_assume(nk >= P::MIN_NK);                   // what the launcher guarantees; the compiler shapes the k-loop's ends by it
    const int wr = wave >> 2, wc = wave & 3;             // wr = the wave's group = its 128-row half; wc = its 64-column strip
    char* const my = smem + wave * 2048;                 // this wave's two pieces of every half-tile
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};

    // ---- prologue: k-tile 0 whole, the B halves of k-tile 1
    if (P::MIN_NK >= 1 || nk > 0) {
        p8_stage<0>(pol, my, 0); p8_stage<1>(pol, my, 0); p8_stage<2>(pol, my, 0); p8_stage<3>(pol, my, 0);
        if (P::MIN_NK >= 2 || nk > 1) { p8_stage<2>(pol, my, 1); p8_stage<3>(pol, my, 1); asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); }
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    p8_sync();
    if (wr == 1) p8_sync();                              // group 1 runs one interval behind

    const int cb0 = (wc & 1) * 4;                        // the wave's first 16-column block inside its B half-tile
    for (int t = 0; t < nk; ++t) {
        const char* sa = smem + (t & 1) * P8_BUF + wr * P8_HALF;
        const char* sb = smem + (t & 1) * P8_BUF + (2 + (wc >> 1)) * P8_HALF;
        bf16x8 afr[2][4], b0[2][2], b1[2][2];
        // ---- phase 0: rows 0-63 × columns 0-31 of the wave tile
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
            for (int j = 0; j < 2; ++j) b0[kb][j] = pol.frag_b(sb, cb0 + j, kb);
#pragma unroll
            for (int i = 0; i < 4; ++i) afr[kb][i] = pol.frag_a(sa, i, kb);
        }
        if (t + 1 < nk) p8_stage<0>(pol, my, t + 1);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        p8_sync();
        __builtin_amdgcn_s_setprio(1);
        p8_mma<P::THREE_TERM, 0, 0>(acc, b0, afr);
        pol.template extra<0>(afr);
        __builtin_amdgcn_s_setprio(0);
        p8_sync();
        // ---- phase 1: rows 0-63 × columns 32-63
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int j = 0; j < 2; ++j) b1[kb][j] = pol.frag_b(sb, cb0 + 2 + j, kb);
        if (t + 1 < nk) p8_stage<1>(pol, my, t + 1);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        p8_sync();
        __builtin_amdgcn_s_setprio(1);
        p8_mma<P::THREE_TERM, 0, 2>(acc, b1, afr);
        __builtin_amdgcn_s_setprio(0);
        p8_sync();
        // ---- phase 2: rows 64-127 × columns 32-63
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int i = 0; i < 4; ++i) afr[kb][i] = pol.frag_a(sa, 4 + i, kb);
        if (t + 2 < nk) p8_stage<2>(pol, my, t + 2);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        p8_sync();
        __builtin_amdgcn_s_setprio(1);
        p8_mma<P::THREE_TERM, 4, 2>(acc, b1, afr);
        pol.template extra<2>(afr);
        __builtin_amdgcn_s_setprio(0);
        p8_sync();
        // ---- phase 3: rows 64-127 × columns 0-31 (fragments already in registers)
        if (t + 2 < nk) p8_stage<3>(pol, my, t + 2);
        if (wr == 1 && t + 1 < nk) p8_wait(t, nk);
        p8_sync();
        __builtin_amdgcn_s_setprio(1);
        p8_mma<P::THREE_TERM, 4, 0>(acc, b0, afr);
        __builtin_amdgcn_s_setprio(0);
        if (wr == 0 && t + 1 < nk) p8_wait(t, nk);
        p8_sync();
    }
    if (wr == 0) p8_sync();                              // both groups pass the same number of barriers: 2 + 8·nk
}

// the two LDS-DMA wave-instructions (1 KiB each, lane-linear) of this wave's share of a half-tile
// (marking the activation loads non-temporal measured 10-25 % slower: the tiles of a tile row share them through L2)
__device__ __forceinline__ void p8_dma2(const __bf16* s0, const __bf16* s1, char* dst) {
    __builtin_amdgcn_global_load_lds((gemm_gptr)(s0), (gemm_lptr)(dst), 16, 0, 0);
    __builtin_amdgcn_global_load_lds((gemm_gptr)(s1), (gemm_lptr)(dst + 1024), 16, 0, 0);
}
// st_16x32 source of this lane: the wave fills the subtiles (row block `wave`, k blocks 0 and 1) of a half-tile that starts at row0; LDS
// slot (row lane>>2, chunk slot lane&3) of a subtile holds logical 16-byte chunk (lane&3) ^ 2·(row >= 8).  Rows past the edge are
// clamped (their sums are never stored).
__device__ __forceinline__ const __bf16* p8_krow_src(const __bf16* X, int ld, int row0, int rows, int wave, int lane) {
    const int sr = lane >> 2, sc = (lane & 3) ^ (((lane >> 5) & 1) << 1);
    return X + (size_t)min(row0 + 16 * wave + sr, rows - 1) * ld + 8 * sc;
}

// One epilogue pass over the wave's 128×64 block: acc (+bias) → the value of mode SV → bf16 → wave-private, XOR-swizzled LDS image
// [128 rows][128 B] → whole-line stores (every global store instruction writes 8 whole 128-byte lines).
enum StoreVal { SV_PRE, SV_ACT, SV_HI = SV_ACT, SV_LO };      // z | act(z) = the hi plane of a split output | its lo plane
template <int ACT, StoreVal SV>
__device__ __forceinline__ void p8_store_pass(const floatx4 (&acc)[8][4], __bf16* __restrict__ C, int ldc, const float4 (&bb)[4], int row0,
                                              int col0, int M, int N, int lane, char* __restrict__ wl) {
    const int l15 = lane & 15, q = lane >> 4;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int r = i * 16 + l15;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float z0 = acc[i][j][0] + bb[j].x, z1 = acc[i][j][1] + bb[j].y, z2 = acc[i][j][2] + bb[j].z, z3 = acc[i][j][3] + bb[j].w;
            if (SV != SV_PRE) { z0 = gemm_act<ACT>(z0); z1 = gemm_act<ACT>(z1); z2 = gemm_act<ACT>(z2); z3 = gemm_act<ACT>(z3); }
            if (SV == SV_LO) { z0 = bf16_lo(z0); z1 = bf16_lo(z1); z2 = bf16_lo(z2); z3 = bf16_lo(z3); }
            uint2 v;
            v.x = pack2(z0, z1); v.y = pack2(z2, z3);
            const int c16 = j * 2 + (q >> 1);           // 16-byte chunk of the row; this lane's 8 bytes are its half (q & 1)
            *reinterpret_cast<uint2*>(wl + r * 128 + ((c16 ^ (r & 7)) << 4) + ((q & 1) << 3)) = v;
        }
        __builtin_amdgcn_sched_barrier(0);              // one row block at a time: keeps the register footprint of the tail small
    }
    // same wave wrote and reads: LDS operations of a wave complete in order.  Global addresses as ONE 32-bit byte offset per lane
    // from the uniform base (host check: the output spans < 4 GiB) stepped by a uniform stride — 16 precomputed 64-bit
    // addresses would not fit beside the 128 accumulator registers a later pass still needs.
    const int chunk = lane & 7, cc = col0 + 8 * chunk, r0 = lane >> 3;
    uint32_t off = ((uint32_t)(row0 + r0) * (uint32_t)ldc + (uint32_t)cc) * 2u;
    const uint32_t step = 16u * (uint32_t)ldc;                         // 8 rows
    const bool col_ok = cc + 8 <= N;
#pragma unroll
    for (int it = 0; it < 16; ++it) {
        const int r = it * 8 + r0;
        const uint4 v = *reinterpret_cast<const uint4*>(wl + r * 128 + ((chunk ^ (r & 7)) << 4));
        if (col_ok && row0 + r < M) *reinterpret_cast<uint4*>(reinterpret_cast<char*>(C) + off) = v;
        off += step;
        if ((it & 3) == 3) __builtin_amdgcn_sched_barrier(0);      // four lines in flight
    }
}
// the bias of the four 16-column blocks of a wave's strip, as a lane holds them (columns 4·(lane>>4) … + 3 of each)
__device__ __forceinline__ void p8_load_bias(float4 (&bb)[4], const float* __restrict__ bias, int col0, int N, int lane) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = col0 + j * 16 + 4 * (lane >> 4);
        bb[j] = (bias && c + 4 <= N) ? *reinterpret_cast<const float4*>(bias + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}
