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

// ---- contrastive decoding (Li et al. 2023; O'Brien & Lewis 2023): an expert's scores held against an amateur's.  The rule, restated by
// tests/contrast_decode_reference.py::combine, row r with C = row_c[r / rows_per] columns, fp64 we > 0, wa ≥ 0, α in [0, 1]; UNK is left
// out of every maximum, head and sum in BOTH score modes and out[UNK] = 0:
//   1. member log-probabilities, fp64, c < C, c ≠ UNK: probability mode p = raw > 0 ? (double)raw : 0 and l = log p (−inf at 0); logits
//      mode l = (double)raw − lse, lse as above; a member row without a finite non-UNK logit is dead: l = −inf everywhere;
//   2. a dead expert row (no column with l_e > −inf): the whole output row is 0;
//   3. head H: probability mode p_e,c > 0 and p_e,c ≥ α·p_e,top (one rounded fp64 product); logits mode raw_e,c finite and
//      (double)raw_e,c − (double)raw_e,top ≥ log α (log α from the host, −inf for α = 0) — only an exact maximum: bit-reproducible;
//   4. amateur term la_c = max(l_a,c, L0), L0 = log(1e-30); with wa == 0 the amateur matrix is never read;
//   5. score s_c = we·l_e,c − wa·la_c, the two products and the difference each rounded, never contracted;
//   6. m = max_H s, Z = Σ_H exp(s_c − m), out_c = fp32(exp((s_c − m) − log Z)) for c in H — a head of one column gives exactly 1.0;
//   7. columns outside H, UNK and C ≤ c < ld_out are 0.
// Three sweeps over a row: (1) the members' log-sum-exps (logits mode) and the expert's maximum, (2) an online (m, Z) over the head,
// (3) the write.  Sweeps 2 and 3 both form s_c (probability mode: two fp64 logs per head column each time; logits mode: none) — the
// widest row would need 64 fp64 registers per lane to keep them.
constexpr double kContrastFloor = -69.07755278982137;      // L0 = log(1e-30)

struct ContrastArgs {
    const float* e; const float* a; int ld_e; int ld_a; double we; double wa; double alpha; double log_alpha;
    const int* row_c; int rows_per; int n_rows; int max_c; int unk;
    float* out; int ld_out;
};

template <int CTRL>
__device__ __forceinline__ double ens_dpp_max_d(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, true);
    return fmax(v, __hiloint2double(hi, lo));
}
__device__ __forceinline__ double ens_wave_max_d(double v) {
    v = ens_dpp_max_d<0xB1>(v);
    v = ens_dpp_max_d<0x4E>(v);
    v = ens_dpp_max_d<0x141>(v);
    v = ens_dpp_max_d<0x140>(v);
    return fmax(fmax(ens_readlane_d(v, 0), ens_readlane_d(v, 16)), fmax(ens_readlane_d(v, 32), ens_readlane_d(v, 48)));
}

// one member row's (maximum, log-sum-exp) over the columns c < C, c ≠ unk: the pass ensemble_combine_kernel takes (all lanes leave the
// loop before the cross-lane steps)
__device__ __forceinline__ void contrast_lse(const float* __restrict__ row, int C, int unk, int lane, float& top, double& lse) {
    float mx = -INFINITY;
    double s = 0.0;
    for (int c = lane; c < C; c += 64) {
        const float x = c != unk ? row[c] : -INFINITY;
        const float hi = fmaxf(mx, x), lo = fminf(mx, x);
        const double e = x == -INFINITY ? 0.0 : exp((double)lo - (double)hi);
        s = x > mx ? s * e + 1.0 : s + e;
        mx = hi;
    }
    top = wave_max(mx);
    const double part = mx == -INFINITY ? 0.0 : s * exp((double)mx - (double)top);
    lse = (double)top + log(ens_wave_sum_d(part));
}

// s_c of one head column (steps 1, 4, 5); xa is read by the caller only when AM
template <bool LOGITS, bool AM>
__device__ __forceinline__ double contrast_score(float xe, float xa, double lse_e, double lse_a, bool live_a, const ContrastArgs& k) {
#pragma clang fp contract(off)
    const double le = LOGITS ? (double)xe - lse_e : log((double)xe);
    const double te = k.we * le;
    if constexpr (!AM) return te;
    double la;
    if constexpr (LOGITS) la = live_a ? (double)xa - lse_a : -INFINITY;
    else la = xa > 0.f ? log((double)xa) : -INFINITY;
    la = fmax(la, kContrastFloor);
    const double ta = k.wa * la;
    return te - ta;
}

template <bool LOGITS, bool AM>
__global__ __launch_bounds__(kEnsThreads) void contrast_combine_kernel(ContrastArgs k) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * (kEnsThreads / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (r >= k.n_rows) return;                    // (wave-uniform)
    int C = k.row_c[r / k.rows_per];
    C = C < 0 ? 0 : (C > k.max_c ? k.max_c : C);  // (as ens_cols: a bad table entry cannot take a read or write out of bounds)
    float* __restrict__ orow = k.out + (size_t)r * k.ld_out;
    const float* __restrict__ erow = k.e + (size_t)r * k.ld_e;
    const float* __restrict__ arow = AM ? k.a + (size_t)r * k.ld_a : nullptr;
    // sweep 1: the expert's maximum (the raw logit, or the probability), the members' log-sum-exps
    float top;
    double lse_e = 0.0, lse_a = 0.0;
    bool live_a = false;
    if constexpr (LOGITS) {
        contrast_lse(erow, C, k.unk, lane, top, lse_e);
        if constexpr (AM) {
            float top_a;
            contrast_lse(arow, C, k.unk, lane, top_a, lse_a);
            live_a = top_a > -INFINITY;
        }
    } else {
        float mx = 0.f;
        for (int c = lane; c < C; c += 64) mx = fmaxf(mx, c != k.unk ? erow[c] : 0.f);      // (fmaxf drops a negative entry: p = 0)
        top = wave_max(mx);
    }
    const bool live_e = LOGITS ? top > -INFINITY : top > 0.f;
    if (!__builtin_amdgcn_readfirstlane((int)live_e)) {       // (wave-uniform: top is the same in every lane) a dead expert row
        for (int c = lane; c < k.ld_out; c += 64) orow[c] = 0.f;
        return;
    }
    const double bound = LOGITS ? k.log_alpha : k.alpha * (double)top;
    auto in_head = [&](int c, float xe) -> bool {
        if (c >= C || c == k.unk) return false;
        if constexpr (LOGITS) return fabsf(xe) < INFINITY && (double)xe - (double)top >= bound;
        else return xe > 0.f && (double)xe >= bound;
    };
    // sweep 2: every lane's running (m, Z) over its head columns, merged once
    double m = -INFINITY, z = 0.0;
    for (int c = lane; c < C; c += 64) {
        const float xe = erow[c];
        if (in_head(c, xe)) {
            const double s = contrast_score<LOGITS, AM>(xe, AM ? arow[c] : 0.f, lse_e, lse_a, live_a, k);
            if (s > m) { z = z * exp(m - s) + 1.0; m = s; }
            else z += exp(s - m);
        }
    }
    const double m_top = ens_wave_max_d(m);       // (all 64 lanes are back together here; the head holds the top column: m_top is finite)
    const double log_z = log(ens_wave_sum_d(m == -INFINITY ? 0.0 : z * exp(m - m_top)));
    // sweep 3: the write
    for (int c = lane; c < k.ld_out; c += 64) {
        float o = 0.f;
        if (c < C) {
            const float xe = erow[c];
            if (in_head(c, xe)) {
                const double s = contrast_score<LOGITS, AM>(xe, AM ? arow[c] : 0.f, lse_e, lse_a, live_a, k);
                o = (float)exp((s - m_top) - log_z);
            }
        }
        orow[c] = o;
    }
}

}  // namespace

extern "C" {

int svpc_contrast_combine(const float* expert, int ld_e, const float* amateur, int ld_a, double we, double wa, double alpha,
                          double log_alpha, const int* row_c, int rows_per, int n_rows, int max_c, int logits, int unk, float* out,
                          int ld_out, hipStream_t stream) {
    constexpr double kMax = 1.7976931348623157e308;
    SVPC_REQUIRE(max_c >= 1 && max_c <= kEnsColsMax && max_c <= ld_out && max_c <= ld_e,
                 "contrast_combine: row columns must be 1..4096 and within ld_e and ld_out");
    SVPC_REQUIRE(rows_per >= 1, "contrast_combine: rows_per must be >= 1");
    SVPC_REQUIRE(we > 0.0 && we <= kMax, "contrast_combine: the expert's weight must be finite and > 0");
    SVPC_REQUIRE(wa >= 0.0 && wa <= kMax, "contrast_combine: the amateur's weight must be finite and >= 0");
    SVPC_REQUIRE(alpha >= 0.0 && alpha <= 1.0, "contrast_combine: alpha must lie in [0, 1]");
    SVPC_REQUIRE(log_alpha <= 0.0, "contrast_combine: log_alpha must be <= 0 (-inf for alpha = 0)");
    SVPC_REQUIRE(wa == 0.0 || max_c <= ld_a, "contrast_combine: row columns must lie within ld_a");
    if (n_rows == 0) return 0;
    SVPC_REQUIRE(n_rows > 0 && expert != nullptr && row_c != nullptr && out != nullptr, "contrast_combine: rows, expert, row_c and out are required");
    SVPC_REQUIRE(wa == 0.0 || amateur != nullptr, "contrast_combine: the amateur's score matrix is missing");
    SVPC_REQUIRE(((uintptr_t)out & 3) == 0, "contrast_combine: out must be 4-byte aligned");
    ContrastArgs k{};
    k.e = expert; k.a = amateur; k.ld_e = ld_e; k.ld_a = ld_a; k.we = we; k.wa = wa; k.alpha = alpha; k.log_alpha = log_alpha;
    k.row_c = row_c; k.rows_per = rows_per; k.n_rows = n_rows; k.max_c = max_c; k.unk = unk; k.out = out; k.ld_out = ld_out;
    const dim3 grid((n_rows + kEnsThreads / 64 - 1) / (kEnsThreads / 64)), block(kEnsThreads);
    if (logits) {
        if (wa != 0.0) hipLaunchKernelGGL((contrast_combine_kernel<true, true>), grid, block, 0, stream, k);
        else hipLaunchKernelGGL((contrast_combine_kernel<true, false>), grid, block, 0, stream, k);
    } else {
        if (wa != 0.0) hipLaunchKernelGGL((contrast_combine_kernel<false, true>), grid, block, 0, stream, k);
        else hipLaunchKernelGGL((contrast_combine_kernel<false, false>), grid, block, 0, stream, k);
    }
    return svpc_check_launch("contrast_combine");
}

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
