// Ensemble decoding (OpenNMT's EnsembleModel / avg_raw_probs, fairseq's ensemble): M members deliver one score matrix each for the same
// hypothesis rows, and the step kernels see ONE probability matrix that combines them.  Rows are independent: one wave per row, four rows
// per workgroup, no LDS, no barrier; every cross-lane step runs with all 64 lanes active and in a fixed order (deterministic).
//
// The rule (restated by tests/ensemble_reference.py::combine), row r with C = row_c[r / rows_per] columns, members m in ascending order,
// fp64 weights w_m > 0 (a zero-weight member is dropped on the host before the launch and is never read):
//   p_{m,c}  probability mode: raw > 0 ? (double)raw : 0;
//            logits mode: exp((double)raw − lse_m), lse_m = max + log Σ exp(raw − max) over the columns c < C, c ≠ unk (the step kernels'
//            convention); p_{m,unk} = 0; a member row without a finite non-unk logit contributes 0 everywhere;
//   rule 0   ("prob")    out_c = fp32(Σ_m w_m·p_{m,c}) — one fp64 multiply and one fp64 add per term, never contracted into an FMA;
//   rule 1   ("logprob") out_c = fp32(exp(Σ_m w_m·log p_{m,c})), 0 as soon as one member has p = 0; log p is (double)raw − lse_m in logits
//            mode (no exp / log round trip); not renormalised;
//   columns C ≤ c < ld_out are written 0.
// The output is a probability matrix in every mode: the step kernels take it with logits = 0.
//
// Members live in a by-value argument struct and the member loop is unrolled through the template parameter M, so the struct's arrays
// are read with constant indices (scalar registers, no scratch) and a captured decode replays the launch unchanged.
#include "common.h"

#include <cmath>

namespace {

constexpr int kEnsMembersMax = 8;
constexpr int kEnsColsMax = 4096;
constexpr int kEnsThreads = 256;              // four rows per workgroup

struct EnsembleArgs {
    const float* p[kEnsMembersMax]; int ld[kEnsMembersMax]; double w[kEnsMembersMax];
    const int* row_c; int rows_per; int n_rows; int max_c; int unk;
    float* out; int ld_out;
};

// fp64 sum over the 64 lanes, the result in every lane (the DPP steps of wave_sum, common.h, on both halves; fixed order)
template <int CTRL>
__device__ __forceinline__ double ens_dpp_add_d(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, true);
    return v + __hiloint2double(hi, lo);
}
__device__ __forceinline__ double ens_readlane_d(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
__device__ __forceinline__ double ens_wave_sum_d(double v) {
    v = ens_dpp_add_d<0xB1>(v);
    v = ens_dpp_add_d<0x4E>(v);
    v = ens_dpp_add_d<0x141>(v);
    v = ens_dpp_add_d<0x140>(v);
    return (ens_readlane_d(v, 0) + ens_readlane_d(v, 16)) + (ens_readlane_d(v, 32) + ens_readlane_d(v, 48));
}

__device__ __forceinline__ int ens_row(const EnsembleArgs& a) {
    return blockIdx.x * (kEnsThreads / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
}
// the row's column count, clamped into what the launch was checked for (a bad table entry cannot take a read or write out of bounds)
__device__ __forceinline__ int ens_cols(const EnsembleArgs& a, int r) {
    const int c = a.row_c[r / a.rows_per];
    return c < 0 ? 0 : (c > a.max_c ? a.max_c : c);
}

// Σ_m w_m·p_m of one column in probability mode: a separate multiply and add per term (numpy cannot reproduce an FMA)
template <int M>
__device__ __forceinline__ float ens_mean(const float (&v)[M], const EnsembleArgs& a) {
#pragma clang fp contract(off)
    double acc = 0.0;
#pragma unroll
    for (int m = 0; m < M; ++m) {
        const double p = v[m] > 0.f ? (double)v[m] : 0.0;
        const double t = a.w[m] * p;
        acc = acc + t;
    }
    return (float)acc;
}

// ---- the streaming leg: rule 0 in probability mode — no transcendental, no row reduction.  VEC: every member row and the output row have
// the same address modulo 16 bytes (checked on the host: equal pointers and leading dimensions modulo 16 bytes / 4 columns), so after a
// scalar head of 0 … 3 columns the body moves 16 bytes per lane and matrix; the tail and the padding columns are scalar.
template <int M, bool VEC>
__global__ __launch_bounds__(kEnsThreads) void ensemble_mean_kernel(EnsembleArgs a) {
    const int lane = threadIdx.x & 63;
    const int r = ens_row(a);
    if (r >= a.n_rows) return;                    // (wave-uniform)
    const int C = ens_cols(a, r);
    float* __restrict__ orow = a.out + (size_t)r * a.ld_out;
    const float* row[M];
#pragma unroll
    for (int m = 0; m < M; ++m) row[m] = a.p[m] + (size_t)r * a.ld[m];
    int c_lo = 0, c_hi = 0;                       // the 16-byte body covers the columns [c_lo, c_hi)
    if constexpr (VEC) {
        const int head = (4 - (int)(((uintptr_t)orow >> 2) & 3)) & 3;
        c_lo = head < C ? head : C;
        c_hi = c_lo + ((C - c_lo) & ~3);
        for (int c = c_lo + 4 * lane; c < c_hi; c += 4 * 64) {
            float4 v[M];
#pragma unroll
            for (int m = 0; m < M; ++m) v[m] = *reinterpret_cast<const float4*>(row[m] + c);
            float x[M], y[M], z[M], w[M];
#pragma unroll
            for (int m = 0; m < M; ++m) { x[m] = v[m].x; y[m] = v[m].y; z[m] = v[m].z; w[m] = v[m].w; }
            *reinterpret_cast<float4*>(orow + c) = make_float4(ens_mean<M>(x, a), ens_mean<M>(y, a), ens_mean<M>(z, a), ens_mean<M>(w, a));
        }
        for (int c = lane; c < c_lo; c += 64) {
            float x[M];
#pragma unroll
            for (int m = 0; m < M; ++m) x[m] = row[m][c];
            orow[c] = ens_mean<M>(x, a);
        }
    }
    for (int c = c_hi + lane; c < a.ld_out; c += 64) {
        float o = 0.f;
        if (c < C) {
            float x[M];
#pragma unroll
            for (int m = 0; m < M; ++m) x[m] = row[m][c];
            o = ens_mean<M>(x, a);
        }
        orow[c] = o;
    }
}

// ---- the other legs: logits mode (either rule) and rule 1 in probability mode — fp64 exp / log per element and member.  Logits mode
// first takes every member's log-sum-exp in ONE pass over its row: each lane keeps a running (maximum, Σ exp(x − maximum)) of its
// columns, the 64 pairs are merged once.  Then one pass over the columns: rule 0 one exp per member, rule 1 no log in logits mode (log p
// is raw − lse) and one exp of the weighted sum.
template <int M, bool LOGITS, int RULE>
__global__ __launch_bounds__(kEnsThreads) void ensemble_combine_kernel(EnsembleArgs a) {
    const int lane = threadIdx.x & 63;
    const int r = ens_row(a);
    if (r >= a.n_rows) return;                    // (wave-uniform)
    const int C = ens_cols(a, r);
    float* __restrict__ orow = a.out + (size_t)r * a.ld_out;
    const float* row[M];
#pragma unroll
    for (int m = 0; m < M; ++m) row[m] = a.p[m] + (size_t)r * a.ld[m];
    double lse[M];
    bool live[M];                                 // (wave-uniform) the member row has a finite non-unk logit
    if constexpr (LOGITS) {
#pragma unroll
        for (int m = 0; m < M; ++m) {
            float mx = -INFINITY;
            double s = 0.0;
            for (int c = lane; c < C; c += 64) {
                const float x = c != a.unk ? row[m][c] : -INFINITY;
                const float hi = fmaxf(mx, x), lo = fminf(mx, x);
                const double e = x == -INFINITY ? 0.0 : exp((double)lo - (double)hi);     // (mx = −inf, x finite: exp(−inf) = 0)
                s = x > mx ? s * e + 1.0 : s + e;
                mx = hi;
            }
            const float top = wave_max(mx);       // (all 64 lanes are back together here)
            const double part = mx == -INFINITY ? 0.0 : s * exp((double)mx - (double)top);
            const double sum = ens_wave_sum_d(part);
            live[m] = top > -INFINITY;
            lse[m] = (double)top + log(sum);
        }
    }
    for (int c = lane; c < a.ld_out; c += 64) {
        float o = 0.f;
        if (c < C && !(LOGITS && c == a.unk)) {
#pragma clang fp contract(off)
            double acc = 0.0;
#pragma unroll
            for (int m = 0; m < M; ++m) {
                const float x = row[m][c];
                double v;
                if constexpr (LOGITS) {
                    const double d = (double)x - lse[m];
                    if constexpr (RULE == 0) v = live[m] ? exp(d) : 0.0;
                    else v = live[m] ? d : -INFINITY;
                } else {
                    v = x > 0.f ? log((double)x) : -INFINITY;       // (rule 1: the streaming kernel has rule 0)
                }
                const double t = a.w[m] * v;
                acc = acc + t;
            }
            o = (float)(RULE == 0 ? acc : exp(acc));
        }
        orow[c] = o;
    }
}

template <int M>
void ens_launch(const EnsembleArgs& a, int logits, int rule, bool vec, hipStream_t stream) {
    const dim3 grid((a.n_rows + kEnsThreads / 64 - 1) / (kEnsThreads / 64)), block(kEnsThreads);
    if (!logits && rule == 0) {
        if (vec) hipLaunchKernelGGL((ensemble_mean_kernel<M, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((ensemble_mean_kernel<M, false>), grid, block, 0, stream, a);
    } else if (!logits) {
        hipLaunchKernelGGL((ensemble_combine_kernel<M, false, 1>), grid, block, 0, stream, a);
    } else if (rule == 0) {
        hipLaunchKernelGGL((ensemble_combine_kernel<M, true, 0>), grid, block, 0, stream, a);
    } else {
        hipLaunchKernelGGL((ensemble_combine_kernel<M, true, 1>), grid, block, 0, stream, a);
    }
}

}  // namespace

extern "C" {

int svpc_ensemble_combine(const float* const* scores, const int* ld, const double* weights, int n_members, const int* row_c, int rows_per,
                          int n_rows, int max_c, int logits, int unk, int rule, float* out, int ld_out, hipStream_t stream) {
    SVPC_REQUIRE(n_members >= 1 && n_members <= kEnsMembersMax, "ensemble_combine: 1..8 members");
    SVPC_REQUIRE(scores != nullptr && ld != nullptr && weights != nullptr, "ensemble_combine: the member tables are required");
    SVPC_REQUIRE(max_c >= 1 && max_c <= kEnsColsMax && max_c <= ld_out, "ensemble_combine: row columns must be 1..4096 and within ld_out");
    SVPC_REQUIRE(rows_per >= 1, "ensemble_combine: rows_per must be >= 1");
    SVPC_REQUIRE(rule == 0 || rule == 1, "ensemble_combine: rule must be 0 (prob) or 1 (logprob)");
    EnsembleArgs a{};
    int n = 0;
    bool vec = true;
    for (int m = 0; m < n_members; ++m) {
        SVPC_REQUIRE(max_c <= ld[m], "ensemble_combine: row columns must lie within every member's ld");
        SVPC_REQUIRE(weights[m] >= 0.0 && weights[m] <= 1.7976931348623157e308, "ensemble_combine: weights must be finite and >= 0");
        if (weights[m] == 0.0) continue;          // a zero-weight member is skipped entirely: it can never produce 0·(−inf)
        SVPC_REQUIRE(scores[m] != nullptr, "ensemble_combine: a member's score matrix is missing");
        a.p[n] = scores[m]; a.ld[n] = ld[m]; a.w[n] = weights[m];
        // 16-byte body: the member's rows sit at the output rows' address modulo 16 bytes
        vec = vec && ((uintptr_t)scores[m] & 15) == ((uintptr_t)out & 15) && (ld[m] - ld_out) % 4 == 0;
        ++n;
    }
    SVPC_REQUIRE(n >= 1, "ensemble_combine: at least one weight must be > 0");
    if (n_rows == 0) return 0;
    SVPC_REQUIRE(n_rows > 0 && row_c != nullptr && out != nullptr, "ensemble_combine: rows, row_c and out are required");
    SVPC_REQUIRE(((uintptr_t)out & 3) == 0, "ensemble_combine: out must be 4-byte aligned");
    a.row_c = row_c; a.rows_per = rows_per; a.n_rows = n_rows; a.max_c = max_c; a.unk = unk; a.out = out; a.ld_out = ld_out;
    switch (n) {
        case 1: ens_launch<1>(a, logits, rule, vec, stream); break;
        case 2: ens_launch<2>(a, logits, rule, vec, stream); break;
        case 3: ens_launch<3>(a, logits, rule, vec, stream); break;
        case 4: ens_launch<4>(a, logits, rule, vec, stream); break;
        case 5: ens_launch<5>(a, logits, rule, vec, stream); break;
        case 6: ens_launch<6>(a, logits, rule, vec, stream); break;
        case 7: ens_launch<7>(a, logits, rule, vec, stream); break;
        default: ens_launch<8>(a, logits, rule, vec, stream); break;
    }
    return svpc_check_launch("ensemble_combine");
}

}  // extern "C"
