// Sequence log-likelihood of GIVEN captions as a training loss (self-critical sequence training): the forward is forced
// decoding's scorer (force.hip) reduced to what a loss needs, the backward the dense gradient of the score matrix, and a small kernel turns
// per-video rewards into per-caption weights.  Layout as force.hip: n_cap caption rows of lt positions, score row r·lt + i scores position
// p = i + 1 of caption r, i = 0 … lt − 2; a caption's scored positions are i < len[r] (svpc_force_inputs).  Restated by
// tests/scst_reference.py.
//
//   svpc_seq_nll_fwd    three launches.  (1) one wave per score row (r, i), i < len[r], four rows per workgroup: the step score of the
//                       target column through score_row.h (log p, −inf for p <= 0; or logit − the fp64 log-sum-exp of the row without
//                       UNK, in beam.hip's order), −inf for a target that is no candidate; rows past the end return before any column
//                       work.  (2) one thread per caption: cum = fp32(cum + step) in position order, barred = a scored position whose
//                       step is not finite, step past the end set to 0.  (3) one workgroup: loss = fp32(−Σ w_r·cum_r) over the captions
//                       that are not barred, products and sums in fp64, thread t its rows t, t + 256, … in order, then a fixed tree.
//   svpc_seq_nll_bwd    one wave per row of the (n_cap·lt, ld_out) gradient, EVERY element written: zero for the columns from C_r up,
//                       the last position row of a caption, the rows past its end and every row of a barred caption; otherwise
//                       −dl·w_r / p at the target column (probabilities), or dl·w_r·(softmax without UNK − [c = y]) with 0 at UNK (logits).
//   svpc_scst_weights   one thread per caption row (and per advantage): A[b, k] = r[b, k] − baseline, w[t·K + k] = fp32(A[vid(t), k] / (N·K)).
//
// Nothing allocates or synchronises; every launch is capturable.
#include "common.h"
#include "score_row.h"

#include <climits>

namespace {

constexpr int kNllThreads = 256;               // four score rows per workgroup

__device__ __forceinline__ bool nll_candidate(int w, int C, int unk) { return w >= 0 && w < C && w != unk; }
__device__ __forceinline__ bool nll_finite(float v) { return v - v == 0.f; }

template <bool LOGITS>
__global__ __launch_bounds__(kNllThreads) void seq_nll_step_kernel(const float* __restrict__ scores, int ld, const int* __restrict__ row_c,
                                                                   const int* __restrict__ tgt, const int* __restrict__ len, int n_cap,
                                                                   int lt, int unk, float* __restrict__ step) {
    const int lane = threadIdx.x & 63;
    const long long g = (long long)blockIdx.x * (kNllThreads / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int steps = lt - 1;
    if (g >= (long long)n_cap * steps) return;    // (wave-uniform)
    const int r = (int)(g / steps), i = (int)(g - (long long)r * steps);
    if (i >= len[r]) return;                      // (wave-uniform) past the caption's end: the finish kernel writes the entry
    const int C = row_c[r];
    const int w = tgt[(size_t)r * lt + i + 1];
    float s = -INFINITY;
    if (nll_candidate(w, C, unk)) {               // (wave-uniform)
        const float* row = scores + ((size_t)r * lt + i) * ld;
        double lse = 0.0;
        if (LOGITS) lse = row_lse(row, C, unk, lane);
        s = step_score(row[w], LOGITS ? 1 : 0, lse);
    }
    if (lane == 0) step[(size_t)r * steps + i] = s;
}

__global__ __launch_bounds__(256) void seq_nll_finish_kernel(const int* __restrict__ len, int n_cap, int lt, float* __restrict__ step,
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
            bar |= nll_finite(s) ? 0 : 1;
        } else {
            step[o] = 0.f;
        }
    }
    cum[r] = cu;
    barred[r] = bar;
}

__global__ __launch_bounds__(256) void seq_nll_loss_kernel(const float* __restrict__ cum, const int* __restrict__ barred,
                                                           const float* __restrict__ row_w, int n_cap, float* __restrict__ loss) {
    __shared__ double part[256];
    double v = 0.0;
    for (int r = threadIdx.x; r < n_cap; r += 256)
        if (!barred[r]) v += (double)row_w[r] * (double)cum[r];
    part[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = (float)(-part[0]);
}

template <bool LOGITS>
__global__ __launch_bounds__(kNllThreads) void seq_nll_bwd_kernel(const float* __restrict__ scores, int ld, const int* __restrict__ row_c,
                                                                  const int* __restrict__ tgt, const int* __restrict__ len,
                                                                  const int* __restrict__ barred, const float* __restrict__ row_w,
                                                                  const float* __restrict__ dl, int n_cap, int lt, int unk,
                                                                  float* __restrict__ dscores, int ld_out) {
    const int lane = threadIdx.x & 63;
    const long long g = (long long)blockIdx.x * (kNllThreads / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (g >= (long long)n_cap * lt) return;       // (wave-uniform)
    const int r = (int)(g / lt), i = (int)(g - (long long)r * lt);
    float* out = dscores + (size_t)g * ld_out;
    const int C = row_c[r];
    const int w = i + 1 < lt ? tgt[(size_t)r * lt + i + 1] : -1;
    // (wave-uniform) a scored position of a caption that is not barred has a candidate target of finite step score
    if (i >= lt - 1 || i >= len[r] || barred[r] || !nll_candidate(w, C, unk)) {
        for (int c = lane; c < ld_out; c += 64) out[c] = 0.f;
        return;
    }
    const float* row = scores + (size_t)g * ld;
    const double s = (double)dl[0] * (double)row_w[r];
    if (LOGITS) {
        const double lse = row_lse(row, C, unk, lane);
        for (int c = lane; c < ld_out; c += 64) {
            float d = 0.f;
            if (c < C && c != unk) d = (float)(s * (exp((double)row[c] - lse) - (c == w ? 1.0 : 0.0)));
            out[c] = d;
        }
    } else {
        const float d = (float)(-s / (double)row[w]);
        for (int c = lane; c < ld_out; c += 64) out[c] = c == w ? d : 0.f;
    }
}

__device__ __forceinline__ double scst_advantage(const double* __restrict__ reward, const double* __restrict__ greedy, int b, int k, int K,
                                                 int rule) {
    const double r = reward[(size_t)b * K + k];
    if (rule == 1) return r - greedy[b];
    if (rule == 2) {
        double sum = 0.0;
        for (int j = 0; j < K; ++j)
            if (j != k) sum += reward[(size_t)b * K + j];
        return r - sum / (double)(K - 1);
    }
    return r;
}

__global__ __launch_bounds__(256) void scst_weights_kernel(const double* __restrict__ reward, const double* __restrict__ greedy,
                                                           const int* __restrict__ row_vid, int n_vid, int K, int n_sent, int rule,
                                                           double* __restrict__ advantage, float* __restrict__ w) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n_vid * K) advantage[j] = scst_advantage(reward, greedy, j / K, j % K, K, rule);
    if (j < n_sent * K) {
        const int b = row_vid[j / K];
        w[j] = (b >= 0 && b < n_vid) ? (float)(scst_advantage(reward, greedy, b, j % K, K, rule) / ((double)n_vid * (double)K)) : 0.f;
    }
}

}  // namespace

extern "C" {

int svpc_seq_nll_fwd(const float* scores, int ld, const int* row_c, int max_c, const int* tgt, const int* len, const float* row_w,
                     int n_cap, int lt, int logits, int unk, float* step, float* cum, int* barred, float* loss, hipStream_t stream) {
    SVPC_REQUIRE(n_cap >= 0 && lt >= 2, "seq_nll_fwd: caption rows of at least two positions");
    if (n_cap > 0) {
        SVPC_REQUIRE(max_c >= 1 && max_c <= ld, "seq_nll_fwd: a row's columns must lie inside the score matrix");
        const long long waves = (long long)n_cap * (lt - 1);
        const long long blocks = (waves + kNllThreads / 64 - 1) / (kNllThreads / 64);
        SVPC_REQUIRE(blocks <= INT_MAX, "seq_nll_fwd: too many score rows for one launch");
        const dim3 grid((unsigned)blocks), block(kNllThreads);
        if (logits)
            hipLaunchKernelGGL(seq_nll_step_kernel<true>, grid, block, 0, stream, scores, ld, row_c, tgt, len, n_cap, lt, unk, step);
        else
            hipLaunchKernelGGL(seq_nll_step_kernel<false>, grid, block, 0, stream, scores, ld, row_c, tgt, len, n_cap, lt, unk, step);
        hipLaunchKernelGGL(seq_nll_finish_kernel, dim3((n_cap + 255) / 256), dim3(256), 0, stream, len, n_cap, lt, step, cum, barred);
    }
    hipLaunchKernelGGL(seq_nll_loss_kernel, dim3(1), dim3(256), 0, stream, cum, barred, row_w, n_cap, loss);
    return svpc_check_launch("seq_nll_fwd");
}

int svpc_seq_nll_bwd(const float* scores, int ld, const int* row_c, int max_c, const int* tgt, const int* len, const int* barred,
                     const float* row_w, const float* dl, int n_cap, int lt, int logits, int unk, float* dscores, int ld_out,
                     hipStream_t stream) {
    if (n_cap == 0) return 0;
    SVPC_REQUIRE(n_cap > 0 && lt >= 2, "seq_nll_bwd: caption rows of at least two positions");
    SVPC_REQUIRE(max_c >= 1 && max_c <= ld && ld_out >= 1, "seq_nll_bwd: a row's columns must lie inside the score matrix");
    const long long waves = (long long)n_cap * lt;
    const long long blocks = (waves + kNllThreads / 64 - 1) / (kNllThreads / 64);
    SVPC_REQUIRE(blocks <= INT_MAX, "seq_nll_bwd: too many score rows for one launch");
    const dim3 grid((unsigned)blocks), block(kNllThreads);
    if (logits)
        hipLaunchKernelGGL(seq_nll_bwd_kernel<true>, grid, block, 0, stream, scores, ld, row_c, tgt, len, barred, row_w, dl, n_cap, lt, unk,
                           dscores, ld_out);
    else
        hipLaunchKernelGGL(seq_nll_bwd_kernel<false>, grid, block, 0, stream, scores, ld, row_c, tgt, len, barred, row_w, dl, n_cap, lt, unk,
                           dscores, ld_out);
    return svpc_check_launch("seq_nll_bwd");
}

int svpc_scst_weights(const double* reward, const double* greedy, const int* row_vid, int n_vid, int k, int n_sent, int rule,
                      double* advantage, float* w, hipStream_t stream) {
    SVPC_REQUIRE(n_vid >= 0 && n_sent >= 0 && k >= 1 && k <= 16, "scst_weights: 1..16 captions per sentence");
    SVPC_REQUIRE(rule >= 0 && rule <= 2, "scst_weights: baseline rule 0 (none), 1 (greedy) or 2 (leave-one-out mean)");
    SVPC_REQUIRE(rule != 1 || greedy != nullptr, "scst_weights: the greedy baseline needs the greedy rewards");
    SVPC_REQUIRE(rule != 2 || k >= 2, "scst_weights: the leave-one-out mean needs K >= 2");
    const int n = (n_vid > n_sent ? n_vid : n_sent) * k;
    if (n == 0) return 0;
    hipLaunchKernelGGL(scst_weights_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, reward, greedy, row_vid, n_vid, k, n_sent, rule,
                       advantage, w);
    return svpc_check_launch("scst_weights");
}

}  // extern "C"
