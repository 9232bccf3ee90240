// Contrastive (SimCTG) training loss on the decoder's last-layer hidden states (Su et al. 2022, "A Contrastive Framework for Neural Text
// Generation"): the training counterpart of contrastive search (contrastive.hip).  Layout as seq_nll.hip: n_cap caption rows
// of lt positions, hidden row r·lt + i (d floats, row stride ld_h) is h_i of caption r; the caption's token set is positions 0 … len[r]
// (svpc_force_inputs' length, clamped into [0, lt − 1] here), n = len[r] + 1 — the history entries contrastive search commits for it.
// Restated by tests/simctg_reference.py.  With rho the margin, in fp64:
//   q_i = |h_i|², dot products in contrastive.hip's order (per lane the elements lane, lane + 64, …, then wave_sum_d's butterfly), so a
//         q_i has the bits contrastive search stores in hist_n2;
//   c_ij = h_i·h_j / (sqrt(q_i)·sqrt(q_j)), 0 when either norm is 0;  m_ij = (rho − 1) + c_ij;  the pair is ACTIVE iff m_ij > 0;
//   cl_r = Σ_{i≠j} max(0, m_ij) / (n(n − 1)),  sim_r = Σ_{i≠j} c_ij / (n(n − 1)),  nact_r = the active ordered pairs;  all 0 for n < 2;
//   loss = fp32(Σ_r v_r·cl_r), products and sums in fp64 in seq_nll_fwd's order (thread t its rows t, t + 256, …, then a fixed tree);
//   d loss / d h_i = dl·v_r·(2 / (n(n − 1)))·(g_i − (g_i·u_i)·u_i) / sqrt(q_i),  u_i = h_i / sqrt(q_i) (0 for a zero row),
//         g_i = Σ_{j : (i, j) active} u_j, g_i·u_i = Σ_{j active} c_ij;  0 for a zero row, for positions > len[r] and for n < 2.
//
// One 256-thread workgroup per caption, in both directions:
//   phase 1: the caption's n rows of d floats → LDS, a wave per row (loaded once, not once per pair);
//   phase 2: the n(n + 1)/2 pairs (i, j ≥ i) dealt to the four waves, four pairs at a time so that their LDS loads and butterflies are
//            independent chains (a short batch repeats its last pair: the same value is stored again) → the Gram matrix in LDS;
//   phase 3: one thread per matrix entry turns the dot product into the cosine in place; one thread per row i sums the row's hinge
//            terms and cosines over j in ascending order and builds the row's mask of active partners;
//   forward: one thread adds the ≤ 32 row sums in ascending order and writes cl, sim, nact; the q_i go out with zeros past the end;
//   backward: recomputes phases 1 … 3 (nothing is saved beside the hidden rows the gradient needs anyway) and then a wave per position
//            row writes EVERY element of its (ld_out wide) gradient row, walking the row's active partners in ascending order.
// n, the pair a wave works on and a row's mask are wave-uniform, so every cross-lane step runs with all 64 lanes; no atomics: the same
// inputs give the same bits.  Nothing allocates or synchronises; every launch is capturable.
#include "common.h"
#include "score_row.h"

#include <climits>
#include <cmath>

namespace {

constexpr int kClThreads = 256;
constexpr int kClWaves = kClThreads / 64;
constexpr int kClMaxLt = 32;                       // a row's active partners are one 32-bit mask
constexpr int kClBatch = 4;                        // pairs a wave has in flight
constexpr size_t kClRowBytes = 144 * 1024;         // the LDS plan: lt·d·4 bytes of rows behind 9,344 bytes of tables, inside the CU's 160 KB

struct ClTables {
    double g[kClMaxLt][kClMaxLt];                  // the Gram matrix, then the cosines (the diagonal keeps q_i)
    double q[kClMaxLt], isq[kClMaxLt];             // q_i and 1 / sqrt(q_i) (0 for a zero row)
    double hs[kClMaxLt], cs[kClMaxLt];             // per row: Σ_j max(0, m_ij), Σ_j c_ij; backward: hs = Σ_{j active} c_ij = g_i·u_i
    unsigned act[kClMaxLt];                        // per row: bit j = the pair (i, j) is active
};
static_assert(sizeof(ClTables) % 16 == 0 && sizeof(ClTables) + kClRowBytes <= 160 * 1024, "the tables and the rows share the CU's 160 KB");

__device__ __forceinline__ int cl_tokens(const int* __restrict__ len, int r, int lt) { return min(max(len[r], 0), lt - 1) + 1; }

// pair p of the upper triangle with the diagonal, row-major: row i holds the n − i pairs (i, i) … (i, n − 1)
__device__ __forceinline__ void cl_pair(int p, int n, int& i, int& j) {
    i = 0;
    while (p >= n - i) { p -= n - i; ++i; }
    j = i + p;
}

// phases 1 … 3 → t.g (cosines off the diagonal), t.q, t.isq, t.act and the per-row sums; ends behind a barrier
__device__ __forceinline__ void cl_rows_gram(const float* __restrict__ h, int ld_h, int D, int n, double rho, float* rows, ClTables& t) {
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int i = wave; i < n; i += kClWaves) {                       // (wave-uniform)
        const float* src = h + (size_t)i * ld_h;
        for (int d = lane; d < D; d += 64) rows[(size_t)i * D + d] = src[d];
    }
    __syncthreads();
    const int P = n * (n + 1) / 2;
    for (int p0 = wave * kClBatch; p0 < P; p0 += kClWaves * kClBatch) {      // (wave-uniform)
        int pi[kClBatch], pj[kClBatch];
        double s[kClBatch];
#pragma unroll
        for (int b = 0; b < kClBatch; ++b) {
            cl_pair(min(p0 + b, P - 1), n, pi[b], pj[b]);
            s[b] = 0.0;
        }
        for (int d = lane; d < D; d += 64) {
#pragma unroll
            for (int b = 0; b < kClBatch; ++b) s[b] += (double)rows[(size_t)pi[b] * D + d] * (double)rows[(size_t)pj[b] * D + d];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
            for (int b = 0; b < kClBatch; ++b) s[b] += __shfl_xor(s[b], o, 64);
        }
        if (lane == 0) {
#pragma unroll
            for (int b = 0; b < kClBatch; ++b) { t.g[pi[b]][pj[b]] = s[b]; t.g[pj[b]][pi[b]] = s[b]; }
        }
    }
    __syncthreads();
    if (tid < kClMaxLt) {
        const double q = tid < n ? t.g[tid][tid] : 0.0;
        t.q[tid] = q;
        t.isq[tid] = q > 0.0 ? 1.0 / sqrt(q) : 0.0;
    }
    __syncthreads();
    for (int e = tid; e < kClMaxLt * kClMaxLt; e += kClThreads) {
        const int i = e / kClMaxLt, j = e % kClMaxLt;
        if (i < n && j < n && i != j) {
            const double qi = t.q[i], qj = t.q[j];
            t.g[i][j] = (qi > 0.0 && qj > 0.0) ? t.g[i][j] / (sqrt(qi) * sqrt(qj)) : 0.0;
        }
    }
    __syncthreads();
    if (tid < kClMaxLt) {
        double hs = 0.0, cs = 0.0;
        unsigned mask = 0u;
        if (tid < n) {
            for (int j = 0; j < n; ++j) {
                if (j == tid) continue;
                const double c = t.g[tid][j], m = (rho - 1.0) + c;
                cs += c;
                if (m > 0.0) { hs += m; mask |= 1u << j; }
            }
        }
        t.hs[tid] = hs;
        t.cs[tid] = cs;
        t.act[tid] = mask;
    }
    __syncthreads();
}

__global__ __launch_bounds__(kClThreads) void seq_cl_fwd_kernel(const float* __restrict__ hidden, int ld_h, int D, const int* __restrict__ len,
                                                                int lt, double rho, float* __restrict__ cl, float* __restrict__ sim,
                                                                int* __restrict__ nact, double* __restrict__ q) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cl_smem[];      // the tables, then the caption's rows: all of it dynamic,
    ClTables& t = *reinterpret_cast<ClTables*>(cl_smem);                        // so that the raised limit covers the kernel's whole LDS
    float* cl_rows = reinterpret_cast<float*>(cl_smem + sizeof(ClTables));
    const int r = blockIdx.x, tid = threadIdx.x;
    const int n = cl_tokens(len, r, lt);           // (workgroup-uniform)
    cl_rows_gram(hidden + (size_t)r * lt * ld_h, ld_h, D, n, rho, cl_rows, t);
    if (tid < lt) q[(size_t)r * lt + tid] = t.q[tid];
    if (tid == 0) {
        double hs = 0.0, cs = 0.0;
        int na = 0;
        for (int i = 0; i < n; ++i) {
            hs += t.hs[i];
            cs += t.cs[i];
            na += __popc(t.act[i]);
        }
        const double pairs = (double)n * (double)(n - 1);
        cl[r] = n >= 2 ? (float)(hs / pairs) : 0.f;
        sim[r] = n >= 2 ? (float)(cs / pairs) : 0.f;
        nact[r] = n >= 2 ? na : 0;
    }
}

__global__ __launch_bounds__(256) void seq_cl_loss_kernel(const float* __restrict__ cl, const float* __restrict__ row_v, int n_cap,
                                                          float* __restrict__ loss) {
    __shared__ double part[256];
    double v = 0.0;
    for (int r = threadIdx.x; r < n_cap; r += 256) v += (double)row_v[r] * (double)cl[r];
    part[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = (float)part[0];
}

__global__ __launch_bounds__(kClThreads) void seq_cl_bwd_kernel(const float* __restrict__ hidden, int ld_h, int D, const int* __restrict__ len,
                                                                const float* __restrict__ row_v, const float* __restrict__ dl, int lt,
                                                                double rho, float* __restrict__ dh, int ld_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cl_smem[];      // the tables, then the caption's rows: all of it dynamic,
    ClTables& t = *reinterpret_cast<ClTables*>(cl_smem);                        // so that the raised limit covers the kernel's whole LDS
    float* cl_rows = reinterpret_cast<float*>(cl_smem + sizeof(ClTables));
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = cl_tokens(len, r, lt);           // (workgroup-uniform)
    float* out = dh + (size_t)r * lt * ld_out;
    if (n < 2) {                                   // (workgroup-uniform) nothing to push apart: the caption's rows are zero
        for (int i = wave; i < lt; i += kClWaves)
            for (int c = lane; c < ld_out; c += 64) out[(size_t)i * ld_out + c] = 0.f;
        return;
    }
    cl_rows_gram(hidden + (size_t)r * lt * ld_h, ld_h, D, n, rho, cl_rows, t);
    if (tid < kClMaxLt) {                          // a_i = Σ_{j active} c_ij = g_i·u_i, over j in ascending order
        double a = 0.0;
        for (unsigned m = t.act[tid]; m; m &= m - 1u) a += t.g[tid][__ffs(m) - 1];
        t.hs[tid] = a;
    }
    __syncthreads();
    const double s = (double)dl[0] * (double)row_v[r] * (2.0 / ((double)n * (double)(n - 1)));
    for (int i = wave; i < lt; i += kClWaves) {    // (wave-uniform)
        float* o = out + (size_t)i * ld_out;
        const double isq = i < n ? t.isq[i] : 0.0;
        if (!(isq > 0.0)) {                        // (wave-uniform) past the end, or a zero row
            for (int c = lane; c < ld_out; c += 64) o[c] = 0.f;
            continue;
        }
        const unsigned mask = __builtin_amdgcn_readfirstlane(t.act[i]);
        const double a = t.hs[i] * isq;
        for (int c = lane; c < ld_out; c += 64) {
            float v = 0.f;
            if (c < D) {
                double g = 0.0;
                for (unsigned m = mask; m; m &= m - 1u) {
                    const int j = __ffs(m) - 1;
                    g += (double)cl_rows[(size_t)j * D + c] * t.isq[j];
                }
                v = (float)(s * isq * (g - a * (double)cl_rows[(size_t)i * D + c]));
            }
            o[c] = v;
        }
    }
}

int cl_check(const float* hidden, int ld_h, int d, const int* len, const float* row_v, int n_cap, int lt, double margin, size_t* lds) {
    SVPC_REQUIRE(n_cap >= 0, "seq_cl: the caption rows cannot be negative");
    SVPC_REQUIRE(lt >= 2 && lt <= kClMaxLt, "seq_cl: caption rows of 2..32 positions");
    SVPC_REQUIRE(d >= 1 && d <= ld_h, "seq_cl: the hidden size must be >= 1 and within the hidden rows");
    SVPC_REQUIRE((size_t)lt * (size_t)d * sizeof(float) <= kClRowBytes, "seq_cl: a caption's Lt rows of D floats must fit 144 KB of LDS");
    SVPC_REQUIRE(std::isfinite(margin) && margin > 0.0 && margin <= 2.0, "seq_cl: the margin must be a finite number in (0, 2]");
    SVPC_REQUIRE(n_cap == 0 || (hidden != nullptr && len != nullptr && row_v != nullptr),
                 "seq_cl: the hidden rows, the lengths and the weights are required");
    *lds = sizeof(ClTables) + (size_t)lt * (size_t)d * sizeof(float);
    return 0;
}

}  // namespace

extern "C" {

int svpc_seq_cl_fwd(const float* hidden, int ld_h, int d, const int* len, const float* row_v, int n_cap, int lt, double margin, float* cl,
                    float* sim, int* nact, double* q, float* loss, hipStream_t stream) {
    size_t lds = 0;
    if (int e = cl_check(hidden, ld_h, d, len, row_v, n_cap, lt, margin, &lds)) return e;
    SVPC_REQUIRE(loss != nullptr && (n_cap == 0 || (cl != nullptr && sim != nullptr && nact != nullptr && q != nullptr)),
                 "seq_cl_fwd: the output arrays are required");
    if (n_cap > 0) {
        if (lds > 64 * 1024)
            if (int e = svpc_raise_lds_once(reinterpret_cast<const void*>(&seq_cl_fwd_kernel), "seq_cl_fwd")) return e;
        hipLaunchKernelGGL(seq_cl_fwd_kernel, dim3(n_cap), dim3(kClThreads), lds, stream, hidden, ld_h, d, len, lt, margin, cl, sim, nact, q);
    }
    hipLaunchKernelGGL(seq_cl_loss_kernel, dim3(1), dim3(256), 0, stream, cl, row_v, n_cap, loss);
    return svpc_check_launch("seq_cl_fwd");
}

int svpc_seq_cl_bwd(const float* hidden, int ld_h, int d, const int* len, const float* row_v, const float* dl, int n_cap, int lt,
                    double margin, float* dh, int ld_out, hipStream_t stream) {
    if (n_cap == 0) return 0;
    size_t lds = 0;
    if (int e = cl_check(hidden, ld_h, d, len, row_v, n_cap, lt, margin, &lds)) return e;
    SVPC_REQUIRE(dl != nullptr && dh != nullptr, "seq_cl_bwd: the upstream factor and the gradient buffer are required");
    SVPC_REQUIRE(ld_out >= d, "seq_cl_bwd: the gradient rows must hold the hidden size");
    if (lds > 64 * 1024)
        if (int e = svpc_raise_lds_once(reinterpret_cast<const void*>(&seq_cl_bwd_kernel), "seq_cl_bwd")) return e;
    hipLaunchKernelGGL(seq_cl_bwd_kernel, dim3(n_cap), dim3(kClThreads), lds, stream, hidden, ld_h, d, len, row_v, dl, lt, margin, dh, ld_out);
    return svpc_check_launch("seq_cl_bwd");
}

}  // extern "C"
