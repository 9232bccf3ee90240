// Preference optimisation over a video's K candidate paragraphs: DPO (Rafailov et al. 2023) and its label-smoothed form
// cDPO (Mitchell 2023), IPO (Azar et al. 2023), SLiC's hinge (Zhao et al. 2023) and the reference-free, length-normalised SimPO (Meng et
// al. 2024).  On top of seq_nll.hip's −Σ w·cum the loss prefers, pair by pair, the candidate of lower cost under the policy's OWN scores
// held against a frozen reference model's scores of the same captions, so the gradient weights depend on the pass's cum and on ref_cum and
// cannot be handed in from outside.  Layout as seq_risk.hip: caption row r = t·K + k, the sentences of video b are the rows t = vid_off[b]
// … vid_off[b + 1] − 1, candidate paragraph k of a video is row k of each of its sentences.  In fp64, per video b and candidate k:
//   s = Σ_t cum[t, k], s_ref = Σ_t ref_cum[t, k] (0 without a reference) in sentence order, n = max(1, Σ_t len[t, k]);
//   valid: no sentence barred, every ref_cum of its sentences finite, cost[b, k] finite; u = (s − s_ref) / n^length_beta, 0 when invalid;
//   pos(k) = the valid candidates before k in the order (cost ascending, k ascending);
//   pairs "all": every (i, j) of valid candidates with cost_i < cost_j; "extremes": pos(i) = 0 and pos(j) = (valid count) − 1, cost_i < cost_j;
//   d = u_i − u_j, h = β·d − γ; ℓ = −(1 − ε)·lnσ(h) − ε·lnσ(−h) (sigmoid; lnσ(x) = min(x, 0) − log1p(exp(−|x|))), max(0, 1 − h) (hinge) or
//   (d − 1 / (2β))² (ipo); D = ∂ℓ / ∂d; pref[b] = (1 / P_b)·Σ_i Σ_j ℓ (per i the sum over j ascending, then the sums over i ascending);
//   G = (ρ / P_b)·(Σ_{pairs with k as i} D − Σ_{pairs with k as j} D), 0 when invalid or P_b = 0; w_eff[t, k] = fp32(w[t, k] − G / (N·n^length_beta)).
// d loss / d scores is svpc_seq_nll_bwd under w_eff: there is no backward here.  Restated by tests/pref_reference.py.
//
//   svpc_seq_pref_fwd   five launches.  (1) … (3) svpc_seq_nll_fwd itself: step, cum and barred are its bits by construction (the loss it
//                       writes is overwritten by (5)).  (4) one wave per video, four per workgroup, lane k = candidate k: the sums over
//                       the video's sentences, the order position by counting and the K² pair loop through shuffles every lane executes
//                       (the tests on `valid` and on pair membership only select what a lane keeps); EVERY element of pref, reward, valid,
//                       n_pairs, n_correct, margin and of the video's w_eff rows is written.  (5) one workgroup: loss = fp32(−Σ w_r·cum_r +
//                       ρ·Σ pref / N), seq_nll_loss_kernel's order for both sums; with ρ = 0 its bits.
//
// Nothing allocates or synchronises; every launch is capturable.
#include "common.h"

#include <climits>

extern "C" int svpc_seq_nll_fwd(const float* scores, int ld, const int* row_c, int max_c, const int* tgt, const int* len, const float* row_w,
                                int n_cap, int lt, int logits, int unk, float* step, float* cum, int* barred, float* loss,
                                hipStream_t stream);

namespace {

constexpr int kPrefThreads = 256;              // four videos per workgroup
constexpr int kPrefMaxK = 16;
enum { kPrefSigmoid = 0, kPrefHinge = 1, kPrefIpo = 2 };

__device__ __forceinline__ bool pref_finite(float v) { return v - v == 0.f; }
__device__ __forceinline__ bool pref_finite_d(double v) { return v - v == 0.0; }

// the loss ℓ of a pair with score difference d (better − worse) and its derivative D = ∂ℓ / ∂d
__device__ __forceinline__ void pref_pair(double d, double beta, double gamma, double eps, int type, double& l, double& D) {
    const double h = beta * d - gamma;
    if (type == kPrefSigmoid) {                   // (wave-uniform)
        const double e = exp(-fabs(h));           // in (0, 1]
        const double lp = fmin(h, 0.0) - log1p(e);        // ln σ(h)
        const double ln = fmin(-h, 0.0) - log1p(e);       // ln σ(−h)
        const double big = 1.0 / (1.0 + e), small = e / (1.0 + e);
        const double sp = h >= 0.0 ? big : small;         // σ(h)
        const double sn = h >= 0.0 ? small : big;         // σ(−h)
        l = -(1.0 - eps) * lp - eps * ln;
        D = beta * (-(1.0 - eps) * sn + eps * sp);
    } else if (type == kPrefHinge) {
        const double a = 1.0 - h;
        l = a > 0.0 ? a : 0.0;
        D = a > 0.0 ? -beta : 0.0;
    } else {
        const double a = d - 1.0 / (2.0 * beta);
        l = a * a;
        D = 2.0 * a;
    }
}

// One wave per video, lane k = candidate k (the lanes from K up carry an invalid candidate and write nothing).  Every __shfl below sits in
// wave-uniform control flow: the loops run 0 … K − 1 in every lane and the tests on `valid` and on the pair only select what a lane keeps.
__global__ __launch_bounds__(kPrefThreads) void seq_pref_group_kernel(const float* __restrict__ cum, const float* __restrict__ ref_cum,
                                                                      const int* __restrict__ len, const int* __restrict__ barred,
                                                                      const float* __restrict__ row_w, const double* __restrict__ cost,
                                                                      const int* __restrict__ vid_off, int n_vid, int n_sent, int K,
                                                                      double beta, double gamma, double eps, double length_beta, double rho,
                                                                      int type, int extremes, double* __restrict__ pref,
                                                                      double* __restrict__ reward, int* __restrict__ valid_out,
                                                                      int* __restrict__ n_pairs, int* __restrict__ n_correct,
                                                                      double* __restrict__ margin, float* __restrict__ w_eff) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * (kPrefThreads / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (b >= n_vid) return;                       // (wave-uniform)
    const bool mine = lane < K;
    // (wave-uniform) the video's sentences, clamped into the caption rows whatever the table holds
    const int t0 = min(max(vid_off[b], 0), n_sent);
    const int t1 = min(max(vid_off[b + 1], t0), n_sent);
    double s = 0.0, sr = 0.0;
    long long words = 0;
    int bad = 0;
    if (mine)
        for (int t = t0; t < t1; ++t) {
            const size_t r = (size_t)t * K + lane;
            s += (double)cum[r];
            words += len[r];
            bad |= barred[r];
            if (ref_cum != nullptr) {             // (wave-uniform)
                const float rc = ref_cum[r];
                sr += (double)rc;
                bad |= pref_finite(rc) ? 0 : 1;
            }
        }
    const double c = mine ? cost[(size_t)b * K + lane] : 0.0;
    const bool valid = mine && !bad && pref_finite_d(c);
    const double scale = pow((double)(words > 1 ? words : 1), length_beta);      // n^length_beta (0: exactly 1)
    const double u = valid ? (s - sr) / scale : 0.0;

    // pos: the valid candidates before this one in the order (cost ascending, k ascending); nv: the valid candidates
    int pos = 0, nv = 0;
    const int vi = valid ? 1 : 0;
    for (int o = 0; o < K; ++o) {
        const double co = __shfl(c, o, 64);
        const int vo = __shfl(vi, o, 64);
        nv += vo;
        if (valid && vo) pos += (co < c || (co == c && o < lane)) ? 1 : 0;
    }

    // the pairs: this lane as the better candidate i against every j, and as the worse candidate j against every i
    double lsum = 0.0, msum = 0.0, dsum = 0.0;
    int cnt = 0, good = 0;
    for (int o = 0; o < K; ++o) {
        const double co = __shfl(c, o, 64);
        const double uo = __shfl(u, o, 64);
        const int po = __shfl(pos, o, 64);
        const int vo = __shfl(vi, o, 64);
        const bool both = valid && vo;
        const bool as_i = both && c < co && (!extremes || (pos == 0 && po == nv - 1));
        const bool as_j = both && co < c && (!extremes || (po == 0 && pos == nv - 1));
        double l, D, lj, Dj;
        pref_pair(u - uo, beta, gamma, eps, type, l, D);
        pref_pair(uo - u, beta, gamma, eps, type, lj, Dj);
        if (as_i) {
            lsum += l;
            msum += beta * (u - uo);
            dsum += D;
            ++cnt;
            good += (u - uo) > 0.0 ? 1 : 0;
        }
        if (as_j) dsum -= Dj;
    }
    double lt = 0.0, mt = 0.0;
    int P = 0, nc = 0;
    for (int o = 0; o < K; ++o) {
        lt += __shfl(lsum, o, 64);
        mt += __shfl(msum, o, 64);
        P += __shfl(cnt, o, 64);
        nc += __shfl(good, o, 64);
    }

    const double G = (valid && P > 0) ? (rho / (double)P) * dsum : 0.0;
    if (mine) {
        const size_t o = (size_t)b * K + lane;
        reward[o] = beta * u;
        valid_out[o] = vi;
        const double gw = G / ((double)n_vid * scale);
        for (int t = t0; t < t1; ++t) {
            const size_t r = (size_t)t * K + lane;
            w_eff[r] = (float)((double)row_w[r] - gw);
        }
    }
    if (lane == 0) {
        pref[b] = P > 0 ? lt / (double)P : 0.0;
        margin[b] = P > 0 ? mt / (double)P : 0.0;
        n_pairs[b] = P;
        n_correct[b] = nc;
    }
}

// Σ of this thread's value over the workgroup in seq_nll_loss_kernel's tree, result in part[0]
__device__ __forceinline__ double pref_block_sum(double* part, double v) {
    __syncthreads();
    part[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    return part[0];
}

__global__ __launch_bounds__(256) void seq_pref_loss_kernel(const float* __restrict__ cum, const int* __restrict__ barred,
                                                            const float* __restrict__ row_w, int n_cap, const double* __restrict__ pref,
                                                            int n_vid, double rho, float* __restrict__ loss) {
    __shared__ double part[256];
    double v = 0.0, a = 0.0;
    for (int r = threadIdx.x; r < n_cap; r += 256)
        if (!barred[r]) v += (double)row_w[r] * (double)cum[r];
    for (int b = threadIdx.x; b < n_vid; b += 256) a += pref[b];
    const double nll = pref_block_sum(part, v);
    const double sa = pref_block_sum(part, a);
    if (threadIdx.x == 0) {
        double out = -nll;
        if (rho != 0.0 && n_vid > 0) out += rho * sa / (double)n_vid;
        loss[0] = (float)out;
    }
}

}  // namespace

extern "C" {

int svpc_seq_pref_fwd(const float* scores, int ld, const int* row_c, int max_c, const int* tgt, const int* len, const float* row_w,
                      const double* cost, const float* ref_cum, const int* vid_off, int n_vid, int n_sent, int k, int lt, int logits, int unk,
                      double beta, double gamma, double label_smoothing, double length_beta, double pref_weight, int loss_type, int pairs,
                      float* step, float* cum, int* barred, double* pref, double* reward, int* valid, int* n_pairs, int* n_correct,
                      double* margin, float* w_eff, float* loss, hipStream_t stream) {
    SVPC_REQUIRE(n_vid >= 0 && n_sent >= 0 && lt >= 2, "seq_pref_fwd: caption rows of at least two positions");
    SVPC_REQUIRE(k >= 1 && k <= kPrefMaxK, "seq_pref_fwd: 1..16 candidates per sentence (one lane each)");
    SVPC_REQUIRE((long long)n_sent * k <= INT_MAX, "seq_pref_fwd: too many caption rows");
    SVPC_REQUIRE(beta > 0.0 && beta - beta == 0.0, "seq_pref_fwd: beta is finite and positive");
    SVPC_REQUIRE(gamma >= 0.0 && length_beta >= 0.0 && pref_weight >= 0.0 && gamma - gamma == 0.0 && length_beta - length_beta == 0.0 &&
                     pref_weight - pref_weight == 0.0,
                 "seq_pref_fwd: gamma, length_beta and pref_weight are finite and not negative");
    SVPC_REQUIRE(label_smoothing >= 0.0 && label_smoothing < 0.5, "seq_pref_fwd: label_smoothing lies in [0, 0.5)");
    SVPC_REQUIRE(loss_type >= kPrefSigmoid && loss_type <= kPrefIpo, "seq_pref_fwd: loss_type 0 (sigmoid), 1 (hinge) or 2 (ipo)");
    SVPC_REQUIRE(pairs == 0 || pairs == 1, "seq_pref_fwd: pairs 0 (all) or 1 (extremes)");
    SVPC_REQUIRE(loss_type == kPrefSigmoid || label_smoothing == 0.0, "seq_pref_fwd: label_smoothing belongs to the sigmoid loss");
    SVPC_REQUIRE(loss_type != kPrefIpo || gamma == 0.0, "seq_pref_fwd: the ipo loss takes no gamma");
    const int n_cap = n_sent * k;
    // step, cum, barred: svpc_seq_nll_fwd's launches (its row checks too); the loss it writes is overwritten below
    const int rc = svpc_seq_nll_fwd(scores, ld, row_c, max_c, tgt, len, row_w, n_cap, lt, logits, unk, step, cum, barred, loss, stream);
    if (rc != 0) return rc;
    if (n_vid > 0) {
        const dim3 grid((unsigned)((n_vid + kPrefThreads / 64 - 1) / (kPrefThreads / 64))), block(kPrefThreads);
        hipLaunchKernelGGL(seq_pref_group_kernel, grid, block, 0, stream, cum, ref_cum, len, barred, row_w, cost, vid_off, n_vid, n_sent, k,
                           beta, gamma, label_smoothing, length_beta, pref_weight, loss_type, pairs, pref, reward, valid, n_pairs, n_correct,
                           margin, w_eff);
    }
    hipLaunchKernelGGL(seq_pref_loss_kernel, dim3(1), dim3(256), 0, stream, cum, barred, row_w, n_cap, pref, n_vid, pref_weight, loss);
    return svpc_check_launch("seq_pref_fwd");
}

}  // extern "C"
