// Minimum-risk (Shen et al. 2016) and ranking (BRIO, Liu et al. 2022) training over a video's K candidate paragraphs: on
// top of seq_nll.hip's −Σ w·cum the loss compares the candidates of one video with each other under the model's OWN scores, so the
// gradient weights depend on the pass's cum and cannot be handed in from outside.  Layout as seq_nll.hip with K candidates per sentence:
// caption row r = t·K + k, the sentences of video b are the rows t = vid_off[b] … vid_off[b + 1] − 1, candidate paragraph k of a video is
// row k of each of its sentences.  In fp64, per video b and candidate k:
//   s = Σ_t cum[t, k] in sentence order, n = max(1, Σ_t len[t, k]), z = s / n^β (0 when a sentence of the candidate is barred);
//   valid: no sentence barred and cost[b, k] finite; an invalid candidate has Q = 0, joins no pair and has G = 0;
//   Q = exp(α(z − max z)) / Σ_valid …, k ascending; risk[b] = Σ_k Q·cost (0 with no valid candidate);
//   pos(k) = the valid candidates before k in the order (cost ascending, k ascending); the pair (i, j), cost_i < cost_j, is active iff
//   h = z_j − z_i + (pos(j) − pos(i))·λ > 0; rank[b] = Σ_i Σ_j h over the active pairs, j ascending inside i ascending;
//   G = ρ_risk·α·Q_k·Σ_k' Q_k'·(cost_k − cost_k') + ρ_rank·(active pairs with k as j − active pairs with k as i) — the centred form of
//   cost_k − risk[b]: exactly 0 when the costs are equal —, w_eff[t, k] = fp32(w[t, k] − G / (N·n^β)).
// d loss / d scores is svpc_seq_nll_bwd under w_eff: there is no backward here.  Restated by tests/risk_reference.py.
//
//   svpc_seq_risk_fwd   four launches.  (1), (2) svpc_seq_nll_fwd's step-score and finish launches (the same bits, through score_row.h).
//                       (3) one wave per video, four per workgroup, lane k = candidate k: the sums over the video's sentences, the
//                       wave-wide maximum, the ordered sums and the K² pair loop through shuffles every lane executes (the branches on
//                       `valid` stay inside the lanes); EVERY element of risk, rank, Q, z, valid and of the video's w_eff rows is written.
//                       (4) one workgroup: loss = fp32(−Σ w_r·cum_r + (ρ_risk·Σ risk + ρ_rank·Σ rank) / N), seq_nll_loss_kernel's order
//                       for each of the three sums; with ρ_risk = ρ_rank = 0 its bits.
//
// Nothing allocates or synchronises; every launch is capturable.
#include "common.h"
#include "score_row.h"

#include <climits>

namespace {

constexpr int kRiskThreads = 256;              // four score rows (or videos) per workgroup
constexpr int kRiskMaxK = 16;

__device__ __forceinline__ bool risk_candidate(int w, int C, int unk) { return w >= 0 && w < C && w != unk; }
__device__ __forceinline__ bool risk_finite(float v) { return v - v == 0.f; }
__device__ __forceinline__ bool risk_finite_d(double v) { return v - v == 0.0; }

template <bool LOGITS>
__global__ __launch_bounds__(kRiskThreads) void seq_risk_step_kernel(const float* __restrict__ scores, int ld, const int* __restrict__ row_c,
                                                                     const int* __restrict__ tgt, const int* __restrict__ len, int n_cap,
                                                                     int lt, int unk, float* __restrict__ step) {
    const int lane = threadIdx.x & 63;
    const long long g = (long long)blockIdx.x * (kRiskThreads / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int steps = lt - 1;
    if (g >= (long long)n_cap * steps) return;    // (wave-uniform)
    const int r = (int)(g / steps), i = (int)(g - (long long)r * steps);
    if (i >= len[r]) return;                      // (wave-uniform) past the caption's end: the finish kernel writes the entry
    const int C = row_c[r];
    const int w = tgt[(size_t)r * lt + i + 1];
    float s = -INFINITY;
    if (risk_candidate(w, C, unk)) {              // (wave-uniform)
        const float* row = scores + ((size_t)r * lt + i) * ld;
        double lse = 0.0;
        if (LOGITS) lse = row_lse(row, C, unk, lane);
        s = step_score(row[w], LOGITS ? 1 : 0, lse);
    }
    if (lane == 0) step[(size_t)r * steps + i] = s;
}

__global__ __launch_bounds__(256) void seq_risk_finish_kernel(const int* __restrict__ len, int n_cap, int lt, float* __restrict__ step,
                                                              float* __restrict__ cum, int* __restrict__ barred) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_cap) return;
    const int steps = lt - 1, n = len[r];
    float cu = 0.f;
    int bar = 0;
    for (int i = 0; i < steps; ++i) {
        const size_t o = (size_t)r * steps + i;
        if (i < n) {
            const float s = step[o];
            cu = cu + s;
            bar |= risk_finite(s) ? 0 : 1;
        } else {
            step[o] = 0.f;
        }
    }
    cum[r] = cu;
    barred[r] = bar;
}

// One wave per video, lane k = candidate k (the lanes from K up carry an invalid candidate and write nothing).  Every __shfl below sits in
// wave-uniform control flow: the loops run 0 … K − 1 in every lane and the tests on `valid` only select what a lane keeps.
__global__ __launch_bounds__(kRiskThreads) void seq_risk_group_kernel(const float* __restrict__ cum, const int* __restrict__ len,
                                                                      const int* __restrict__ barred, const float* __restrict__ row_w,
                                                                      const double* __restrict__ cost, const int* __restrict__ vid_off,
                                                                      int n_vid, int n_sent, int K, double alpha, double beta, double margin,
                                                                      double rho_risk, double rho_rank, double* __restrict__ risk,
                                                                      double* __restrict__ rank, double* __restrict__ Q,
                                                                      double* __restrict__ z_out, int* __restrict__ valid_out,
                                                                      float* __restrict__ w_eff) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * (kRiskThreads / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (b >= n_vid) return;                       // (wave-uniform)
    const bool mine = lane < K;
    // (wave-uniform) the video's sentences, clamped into the caption rows whatever the table holds
    const int t0 = min(max(vid_off[b], 0), n_sent);
    const int t1 = min(max(vid_off[b + 1], t0), n_sent);
    double s = 0.0;
    long long words = 0;
    int bar = 0;
    if (mine)
        for (int t = t0; t < t1; ++t) {
            const size_t r = (size_t)t * K + lane;
            s += (double)cum[r];
            words += len[r];
            bar |= barred[r];
        }
    const double c = mine ? cost[(size_t)b * K + lane] : 0.0;
    const bool valid = mine && !bar && risk_finite_d(c);
    const double scale = pow((double)(words > 1 ? words : 1), beta);      // n^β (β = 0: exactly 1)
    const double z = bar ? 0.0 : s / scale;

    // Q: the maximum over the valid candidates, then the ordered sums
    const double zmax = wave_max_d(valid ? z : -INFINITY);
    const double e = valid ? exp(alpha * (z - zmax)) : 0.0;
    double den = 0.0;
    for (int o = 0; o < K; ++o) den += __shfl(e, o, 64);
    const double q = valid ? e / den : 0.0;
    const double qc = valid ? q * c : 0.0;
    double rk = 0.0;
    for (int o = 0; o < K; ++o) rk += __shfl(qc, o, 64);

    // pos: the valid candidates before this one in the order (cost ascending, k ascending); dev = Σ_k' Q_k'·(cost − cost_k')
    int pos = 0;
    double dev = 0.0;
    const int vi = valid ? 1 : 0;
    for (int o = 0; o < K; ++o) {
        const double co = __shfl(c, o, 64);
        const double qo = __shfl(q, o, 64);
        const int vo = __shfl(vi, o, 64);
        if (valid && vo) {
            pos += (co < c || (co == c && o < lane)) ? 1 : 0;
            dev += qo * (c - co);
        }
    }

    // the pairs: this lane as the better candidate i against every j, and as the worse candidate j against every i
    double hinge = 0.0;
    int as_i = 0, as_j = 0;
    for (int o = 0; o < K; ++o) {
        const double co = __shfl(c, o, 64);
        const double zo = __shfl(z, o, 64);
        const int po = __shfl(pos, o, 64);
        const int vo = __shfl(vi, o, 64);
        if (valid && vo) {
            if (c < co) {
                const double h = zo - z + (double)(po - pos) * margin;
                if (h > 0.0) {
                    hinge += h;
                    ++as_i;
                }
            }
            if (co < c) {
                const double h = z - zo + (double)(pos - po) * margin;
                if (h > 0.0) ++as_j;
            }
        }
    }
    double rn = 0.0;
    for (int o = 0; o < K; ++o) rn += __shfl(hinge, o, 64);

    const double G = valid ? rho_risk * alpha * q * dev + rho_rank * (double)(as_j - as_i) : 0.0;
    if (mine) {
        const size_t o = (size_t)b * K + lane;
        Q[o] = q;
        z_out[o] = z;
        valid_out[o] = vi;
        const double gw = G / ((double)n_vid * scale);
        for (int t = t0; t < t1; ++t) {
            const size_t r = (size_t)t * K + lane;
            w_eff[r] = (float)((double)row_w[r] - gw);
        }
    }
    if (lane == 0) {
        risk[b] = rk;
        rank[b] = rn;
    }
}

// Σ of this thread's value over the workgroup in seq_nll_loss_kernel's tree, result in part[0]
__device__ __forceinline__ double risk_block_sum(double* part, double v) {
    __syncthreads();
    part[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    return part[0];
}

__global__ __launch_bounds__(256) void seq_risk_loss_kernel(const float* __restrict__ cum, const int* __restrict__ barred,
                                                            const float* __restrict__ row_w, int n_cap, const double* __restrict__ risk,
                                                            const double* __restrict__ rank, int n_vid, double rho_risk, double rho_rank,
                                                            float* __restrict__ loss) {
    __shared__ double part[256];
    double v = 0.0, a = 0.0, c = 0.0;
    for (int r = threadIdx.x; r < n_cap; r += 256)
        if (!barred[r]) v += (double)row_w[r] * (double)cum[r];
    for (int b = threadIdx.x; b < n_vid; b += 256) {
        a += risk[b];
        c += rank[b];
    }
    const double nll = risk_block_sum(part, v);
    const double sa = risk_block_sum(part, a);
    const double sc = risk_block_sum(part, c);
    if (threadIdx.x == 0) {
        double out = -nll;
        if ((rho_risk != 0.0 || rho_rank != 0.0) && n_vid > 0) out += (rho_risk * sa + rho_rank * sc) / (double)n_vid;
        loss[0] = (float)out;
    }
}

}  // namespace

extern "C" {

int svpc_seq_risk_fwd(const float* scores, int ld, const int* row_c, int max_c, const int* tgt, const int* len, const float* row_w,
                      const double* cost, const int* vid_off, int n_vid, int n_sent, int k, int lt, int logits, int unk, double alpha,
                      double length_beta, double margin, double risk_weight, double rank_weight, float* step, float* cum, int* barred,
                      double* risk, double* rank, double* q, double* z, int* valid, float* w_eff, float* loss, hipStream_t stream) {
    SVPC_REQUIRE(n_vid >= 0 && n_sent >= 0 && lt >= 2, "seq_risk_fwd: caption rows of at least two positions");
    SVPC_REQUIRE(k >= 1 && k <= kRiskMaxK, "seq_risk_fwd: 1..16 candidates per sentence (one lane each)");
    SVPC_REQUIRE((long long)n_sent * k <= INT_MAX, "seq_risk_fwd: too many caption rows");
    SVPC_REQUIRE(alpha >= 0.0 && length_beta >= 0.0 && margin >= 0.0 && risk_weight >= 0.0 && rank_weight >= 0.0 && alpha - alpha == 0.0 &&
                     length_beta - length_beta == 0.0 && margin - margin == 0.0 && risk_weight - risk_weight == 0.0 &&
                     rank_weight - rank_weight == 0.0,
                 "seq_risk_fwd: alpha, length_beta, margin and the two weights are finite and not negative");
    const int n_cap = n_sent * k;
    if (n_cap > 0) {
        SVPC_REQUIRE(max_c >= 1 && max_c <= ld, "seq_risk_fwd: a row's columns must lie inside the score matrix");
        const long long waves = (long long)n_cap * (lt - 1);
        const long long blocks = (waves + kRiskThreads / 64 - 1) / (kRiskThreads / 64);
        SVPC_REQUIRE(blocks <= INT_MAX, "seq_risk_fwd: too many score rows for one launch");
        const dim3 grid((unsigned)blocks), block(kRiskThreads);
        if (logits)
            hipLaunchKernelGGL(seq_risk_step_kernel<true>, grid, block, 0, stream, scores, ld, row_c, tgt, len, n_cap, lt, unk, step);
        else
            hipLaunchKernelGGL(seq_risk_step_kernel<false>, grid, block, 0, stream, scores, ld, row_c, tgt, len, n_cap, lt, unk, step);
        hipLaunchKernelGGL(seq_risk_finish_kernel, dim3((n_cap + 255) / 256), dim3(256), 0, stream, len, n_cap, lt, step, cum, barred);
    }
    if (n_vid > 0) {
        const dim3 grid((unsigned)((n_vid + kRiskThreads / 64 - 1) / (kRiskThreads / 64))), block(kRiskThreads);
        hipLaunchKernelGGL(seq_risk_group_kernel, grid, block, 0, stream, cum, len, barred, row_w, cost, vid_off, n_vid, n_sent, k, alpha,
                           length_beta, margin, risk_weight, rank_weight, risk, rank, q, z, valid, w_eff);
    }
    hipLaunchKernelGGL(seq_risk_loss_kernel, dim3(1), dim3(256), 0, stream, cum, barred, row_w, n_cap, risk, rank, n_vid, risk_weight,
                       rank_weight, loss);
    return svpc_check_launch("seq_risk_fwd");
}

}  // extern "C"
