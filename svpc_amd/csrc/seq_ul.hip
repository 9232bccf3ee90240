// Unlikelihood training against repetition (Welleck et al. 2020): on top of seq_nll.hip's −Σ w·log p(caption) the loss
// adds Σ u·ul, ul the sum over a caption's scored positions of −log(1 − p(c)) over that position's NEGATIVE columns c.  Layout as
// seq_nll.hip: n_cap caption rows of lt positions, score row r·lt + i scores position p = i + 1, i = 0 … lt − 2, scored while i < len[r].
// neg (n_cap, lt − 1, M) int32 lists up to M columns per position (−1: none); a listing counts when it is a candidate (0 <= c < C_r,
// c != unk) of a scored position, and a column listed twice counts twice.  In fp64: p_c = row[c] (probabilities) or exp(row[c] − lse)
// (logits), q = 1 − p_c, term = −log1p(−p_c) when q >= kUlEps, else −log kUlEps with a zero gradient (the published implementation's
// clamp).  Restated by tests/unlikelihood_reference.py.
//
//   svpc_ul_negatives   one wave per caption row, one lane per position: the negatives of the "token" rule (M = lt − 1: the distinct
//                       earlier words of the caption in order of first occurrence, without the position's target and non-candidates) or of
//                       the "ngram" rule (M = 1: the word of every position inside an n-gram that repeats an earlier one of the caption
//                       or, under paragraph scope, one of the same candidate row of an earlier sentence of the video), and the counts.
//   svpc_seq_ul_fwd     three launches as svpc_seq_nll_fwd.  (1) one wave per score row (r, i), i < len[r], four per workgroup: the
//                       target's step score through score_row.h (seq_nll.hip's bits) and, lane j carrying listing j, ulstep =
//                       fp32(Σ_j term); rows past the end return before any column work.  (2) one thread per caption: cum, barred, ul =
//                       fp32(ul + ulstep) in position order, zeroes past the end.  (3) one workgroup: loss = fp32(−Σ w_r·cum_r + Σ u_r·ul_r)
//                       over the captions that are not barred, seq_nll_loss_kernel's order.
//   svpc_seq_ul_bwd     one wave per row of the (n_cap·lt, ld_out) gradient, EVERY element written once by the lane that owns its column:
//                       the zero rows and columns of svpc_seq_nll_bwd; else, probabilities, −dl·w / p_y at the target and dl·u / (1 − p_c)
//                       per counted, unclamped listing of c; logits, dl·[w·(p_c − [c = y]) + u·(a_c − A·p_c)], a_c = Σ p_c / (1 − p_c)
//                       over those listings of c, A = Σ_c a_c, 0 at unk.  A row with dl·u = 0 is seq_nll_bwd_kernel's row, bit for bit.
//
// Nothing allocates or synchronises; every launch is capturable.
#include "common.h"
#include "score_row.h"

#include <climits>

namespace {

constexpr int kUlThreads = 256;                // four score rows per workgroup
constexpr double kUlEps = 1e-5;                // the clamp on 1 − p: a defined constant, not a tolerance

__device__ __forceinline__ bool ul_candidate(int w, int C, int unk) { return w >= 0 && w < C && w != unk; }
__device__ __forceinline__ bool ul_finite(float v) { return v - v == 0.f; }

__device__ __forceinline__ int wave_sum_i(int v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ------------------------------------------------------------------------------------------------ the negatives
// Does this lane's gram g (n words) equal one of the grams of a caption whose words 1 … nw are held one per lane (word p in lane p − 1) and
// that starts before position `before`?  The caption's grams are walked in a wave-uniform loop; their words come out of the lanes by
// v_readlane (a uniform index), not out of memory: one load per caption row instead of a chain of dependent loads per gram.
__device__ __forceinline__ bool ul_gram_match(int words, int nw, int n, const int (&g)[4], int before) {
    bool rep = false;
    for (int b = 1; b + n - 1 <= nw; ++b) {       // (wave-uniform)
        bool eq = b < before;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < n) eq = eq && __builtin_amdgcn_readlane(words, b - 1 + j) == g[j];       // (j < n: wave-uniform)
        rep = rep || eq;
    }
    return rep;
}

// RULE 0 "token", 1 "ngram".  Lane l is position p = l + 1 (score row i = l) and, under "ngram", the gram that starts at p.
template <int RULE>
__global__ __launch_bounds__(kUlThreads) void ul_negatives_kernel(const int* __restrict__ tgt, const int* __restrict__ len,
                                                                  const int* __restrict__ finished, const int* __restrict__ row_c, int n_cap,
                                                                  int lt, int unk, int n, int paragraph, const int* __restrict__ sent_first,
                                                                  int K, int* __restrict__ neg, int* __restrict__ npen,
                                                                  int* __restrict__ nrep) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * (kUlThreads / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (r >= n_cap) return;                       // (wave-uniform)
    const int steps = lt - 1;
    const int C = row_c[r];
    const int* y = tgt + (size_t)r * lt;
    const int nl = min(max(len[r], 0), steps);    // (a length outside 0 … lt − 1 reads nothing outside the row)
    const int x = lane < steps ? y[lane + 1] : -1;
    if (RULE == 0) {
        // first[l]: no earlier position holds the word of position l + 1
        bool first = true;
        for (int o = 0; o < steps; ++o) {         // (wave-uniform trip count: every lane takes part in every shuffle)
            const int v = __shfl(x, o, 64);
            if (o < lane && v == x) first = false;
        }
        int cnt = 0;
        int* out = neg + ((size_t)r * steps + lane) * steps;
        for (int o = 0; o < steps; ++o) {         // (wave-uniform trip count)
            const int v = __shfl(x, o, 64);
            const int f = __shfl((int)first, o, 64);
            if (lane < nl && o < lane && f && v != x && ul_candidate(v, C, unk)) out[cnt++] = v;
        }
        if (lane < steps)
            for (int j = cnt; j < steps; ++j) out[j] = -1;
        const int total = wave_sum_i(cnt);
        if (lane == 0) {
            npen[r] = total;
            nrep[r] = 0;
        }
    } else {
        const int nw = max(nl - (finished[r] ? 1 : 0), 0);
        const int a = lane + 1;                   // this lane's gram: words a … a + n − 1
        const bool gram = a + n - 1 <= nw;
        int g[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) g[j] = (j < n && gram) ? y[a + j] : 0;
        // the same caption: an equal gram that starts earlier
        bool rep = ul_gram_match(x, nw, n, g, a);
        // paragraph scope: any gram of the same candidate row of an earlier sentence of the video
        if (paragraph) {                          // (wave-uniform)
            const int t = r / K, k = r - t * K;
            const int t0 = min(max(sent_first[t], 0), t);
            for (int s = t0; s < t; ++s) {        // (wave-uniform)
                const int q = s * K + k;
                const int z = lane < steps ? tgt[(size_t)q * lt + lane + 1] : -1;
                const int nq = max(min(max(len[q], 0), steps) - (finished[q] ? 1 : 0), 0);
                rep = ul_gram_match(z, nq, n, g, INT_MAX) || rep;
            }
        }
        const u64 mask = __ballot(rep && gram);   // bit l: the gram that starts at position l + 1 repeats
        // position p = lane + 1 is penalised when a repeat gram starts at one of p − n + 1 … p, that is at one of the bits lane − n + 1 … lane
        const int lo = max(lane - n + 1, 0);
        const bool pen = lane < steps && ((mask >> lo) & ((1ull << (lane - lo + 1)) - 1ull)) != 0ull;
        if (lane < steps) neg[(size_t)r * steps + lane] = pen ? x : -1;
        const u64 counted = __ballot(pen && ul_candidate(x, C, unk));
        if (lane == 0) {
            npen[r] = __popcll(counted);
            nrep[r] = __popcll(mask);
        }
    }
}

// ------------------------------------------------------------------------------------------------ the forward
// lane j's listing of score row (r, i): the column (−1: not counted), its probability and whether the clamp holds it
struct UlListing {
    int c;
    double p;
    bool live;                                    // counted and 1 − p >= kUlEps: it has a gradient
};

// c: lane j's entry of the row's negatives (−1 for the lanes from M up)
template <bool LOGITS>
__device__ __forceinline__ UlListing ul_listing(const float* __restrict__ row, int c, int C, int unk, double lse) {
    UlListing l{-1, 0.0, false};
    if (ul_candidate(c, C, unk)) {
        l.c = c;
        l.p = LOGITS ? exp((double)row[c] - lse) : (double)row[c];
        l.live = 1.0 - l.p >= kUlEps;
    }
    return l;
}

template <bool LOGITS>
__global__ __launch_bounds__(kUlThreads) void seq_ul_step_kernel(const float* __restrict__ scores, int ld, const int* __restrict__ row_c,
                                                                 const int* __restrict__ tgt, const int* __restrict__ len,
                                                                 const int* __restrict__ neg, int m, int n_cap, int lt, int unk,
                                                                 float* __restrict__ step, float* __restrict__ ulstep) {
    const int lane = threadIdx.x & 63;
    const long long g = (long long)blockIdx.x * (kUlThreads / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int steps = lt - 1;
    if (g >= (long long)n_cap * steps) return;    // (wave-uniform)
    const int r = (int)(g / steps), i = (int)(g - (long long)r * steps);
    if (i >= len[r]) return;                      // (wave-uniform) past the caption's end: the finish kernel writes the entries
    const int C = row_c[r];
    const int w = tgt[(size_t)r * lt + i + 1];
    const float* row = scores + ((size_t)r * lt + i) * ld;
    double lse = 0.0;
    if (LOGITS) lse = row_lse(row, C, unk, lane);
    float s = -INFINITY;
    if (ul_candidate(w, C, unk)) s = step_score(row[w], LOGITS ? 1 : 0, lse);      // (wave-uniform)
    const UlListing l = ul_listing<LOGITS>(row, lane < m ? neg[(size_t)g * m + lane] : -1, C, unk, lse);
    double term = 0.0;
    if (l.c >= 0) term = l.live ? -log1p(-l.p) : -log(kUlEps);
    term = wave_sum_d(term);
    if (lane == 0) {
        step[g] = s;
        ulstep[g] = (float)term;
    }
}

__global__ __launch_bounds__(256) void seq_ul_finish_kernel(const int* __restrict__ len, int n_cap, int lt, float* __restrict__ step,
                                                            float* __restrict__ ulstep, float* __restrict__ cum, float* __restrict__ ul,
                                                            int* __restrict__ barred) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_cap) return;
    const int steps = lt - 1, n = len[r];
    float cu = 0.f, uu = 0.f;
    int bar = 0;
    for (int i = 0; i < steps; ++i) {
        const size_t o = (size_t)r * steps + i;
        if (i < n) {
            const float s = step[o];
            cu = cu + s;
            uu = uu + ulstep[o];
            bar |= ul_finite(s) ? 0 : 1;
        } else {
            step[o] = 0.f;
            ulstep[o] = 0.f;
        }
    }
    cum[r] = cu;
    ul[r] = uu;
    barred[r] = bar;
}

__global__ __launch_bounds__(256) void seq_ul_loss_kernel(const float* __restrict__ cum, const float* __restrict__ ul,
                                                          const int* __restrict__ barred, const float* __restrict__ row_w,
                                                          const float* __restrict__ row_u, int n_cap, float* __restrict__ loss) {
    __shared__ double part[256];
    double v = 0.0;
    for (int r = threadIdx.x; r < n_cap; r += 256)
        if (!barred[r]) {
            v += (double)row_w[r] * (double)cum[r];
            v -= (double)row_u[r] * (double)ul[r];
        }
    part[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = (float)(-part[0]);
}

// ------------------------------------------------------------------------------------------------ the backward
// Σ of coef over the live listings (mask: their lanes, wave-uniform) whose column is c, in lane order: every lane walks the same listings
__device__ __forceinline__ double ul_gather(u64 mask, int lc, double coef, int c) {
    double acc = 0.0;
    while (mask) {                                // (wave-uniform: the mask is a ballot)
        const int j = __builtin_ctzll(mask);
        mask &= mask - 1;
        const int cj = __shfl(lc, j, 64);
        const double gj = __shfl(coef, j, 64);
        if (cj == c) acc += gj;
    }
    return acc;
}

template <bool LOGITS>
__global__ __launch_bounds__(kUlThreads) void seq_ul_bwd_kernel(const float* __restrict__ scores, int ld, const int* __restrict__ row_c,
                                                                const int* __restrict__ tgt, const int* __restrict__ len,
                                                                const int* __restrict__ barred, const int* __restrict__ neg, int m,
                                                                const float* __restrict__ row_w, const float* __restrict__ row_u,
                                                                const float* __restrict__ dl, int n_cap, int lt, int unk,
                                                                float* __restrict__ dscores, int ld_out) {
    const int lane = threadIdx.x & 63;
    const long long g = (long long)blockIdx.x * (kUlThreads / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (g >= (long long)n_cap * lt) return;       // (wave-uniform)
    const int r = (int)(g / lt), i = (int)(g - (long long)r * lt);
    float* out = dscores + (size_t)g * ld_out;
    const int C = row_c[r];
    const int w = i + 1 < lt ? tgt[(size_t)r * lt + i + 1] : -1;
    // lane j's listing, loaded with the row's other tables and not after the zero-row test: the listing's score load waits for it
    // (measured at the training shape: no difference either way)
    const int nc = (i < lt - 1 && lane < m) ? neg[((size_t)r * (lt - 1) + i) * m + lane] : -1;
    // (wave-uniform) a scored position of a caption that is not barred has a candidate target of finite step score
    if (i >= lt - 1 || i >= len[r] || barred[r] || !ul_candidate(w, C, unk)) {
        for (int c = lane; c < ld_out; c += 64) out[c] = 0.f;
        return;
    }
    const float* row = scores + (size_t)g * ld;
    const double s = (double)dl[0] * (double)row_w[r];
    const double su = (double)dl[0] * (double)row_u[r];
    const bool with_u = su != 0.0;                // (wave-uniform) without it the row is seq_nll_bwd_kernel's, bit for bit
    if (LOGITS) {
        const double lse = row_lse(row, C, unk, lane);
        u64 mask = 0ull;
        double coef = 0.0, A = 0.0;
        int lc = -1;
        if (with_u) {                             // (wave-uniform)
            const UlListing l = ul_listing<true>(row, nc, C, unk, lse);
            lc = l.live ? l.c : -1;
            coef = l.live ? l.p / (1.0 - l.p) : 0.0;
            mask = __ballot(l.live);
            A = wave_sum_d(coef);
        }
        for (int c0 = 0; c0 < ld_out; c0 += 64) {
            const int c = c0 + lane;
            // (wave-uniform) the live listings that fall into this chunk of 64 columns; all 64 lanes walk them before the lanes diverge
            const u64 here = mask ? (mask & __ballot(lc >= c0 && lc < c0 + 64)) : 0ull;
            const double a = ul_gather(here, lc, coef, c);
            float d = 0.f;
            if (c < C && c != unk) {
                const double p = exp((double)row[c] - lse);
                double v = s * (p - (c == w ? 1.0 : 0.0));
                if (with_u) v += su * (a - A * p);
                d = (float)v;
            }
            if (c < ld_out) out[c] = d;
        }
    } else {
        const double dw = -s / (double)row[w];
        u64 mask = 0ull;
        double coef = 0.0;
        int lc = -1;
        if (with_u) {                             // (wave-uniform)
            const UlListing l = ul_listing<false>(row, nc, C, unk, 0.0);
            lc = l.live ? l.c : -1;
            coef = l.live ? 1.0 / (1.0 - l.p) : 0.0;
            mask = __ballot(l.live);
        }
        for (int c0 = 0; c0 < ld_out; c0 += 64) {
            const int c = c0 + lane;
            // (wave-uniform) the listings that fall into this chunk of 64 columns; none: the chunk is zeros and the target
            const u64 here = mask ? (mask & __ballot(lc >= c0 && lc < c0 + 64)) : 0ull;
            float d = c == w ? (float)dw : 0.f;
            if (here) {                           // (wave-uniform)
                const double acc = ul_gather(here, lc, coef, c);
                if (acc != 0.0) d = (float)((c == w ? dw : 0.0) + su * acc);        // (a live listing's 1 / (1 − p) is never 0)
            }
            if (c < ld_out) out[c] = d;
        }
    }
}

}  // namespace

extern "C" {

int svpc_ul_negatives(const int* tgt, const int* len, const int* finished, const int* row_c, int n_cap, int lt, int unk, int rule, int ngram,
                      int paragraph, const int* sent_first, int k, int* neg, int* npen, int* nrep, hipStream_t stream) {
    SVPC_REQUIRE(n_cap >= 0 && lt >= 2, "ul_negatives: caption rows of at least two positions");
    SVPC_REQUIRE(lt - 1 <= 64, "ul_negatives: one lane per position, at most 64 scored positions (Lt <= 65)");
    SVPC_REQUIRE(rule == 0 || rule == 1, "ul_negatives: rule 0 (token) or 1 (ngram)");
    SVPC_REQUIRE(rule == 0 || (ngram >= 1 && ngram <= 4), "ul_negatives: n-grams of 1..4 words");
    SVPC_REQUIRE(rule == 0 || !paragraph || (sent_first != nullptr && k >= 1 && n_cap % k == 0),
                 "ul_negatives: paragraph scope needs the sentences' first-sentence table and K dividing the caption rows");
    if (n_cap == 0) return 0;
    const dim3 grid((unsigned)((n_cap + kUlThreads / 64 - 1) / (kUlThreads / 64))), block(kUlThreads);
    if (rule == 0)
        hipLaunchKernelGGL(ul_negatives_kernel<0>, grid, block, 0, stream, tgt, len, finished, row_c, n_cap, lt, unk, 0, 0, sent_first, 1, neg,
                           npen, nrep);
    else
        hipLaunchKernelGGL(ul_negatives_kernel<1>, grid, block, 0, stream, tgt, len, finished, row_c, n_cap, lt, unk, ngram, paragraph ? 1 : 0,
                           sent_first, paragraph ? k : 1, neg, npen, nrep);
    return svpc_check_launch("ul_negatives");
}

int svpc_seq_ul_fwd(const float* scores, int ld, const int* row_c, int max_c, const int* tgt, const int* len, const int* neg, int m,
                    const float* row_w, const float* row_u, int n_cap, int lt, int logits, int unk, float* step, float* ulstep, float* cum,
                    float* ul, int* barred, float* loss, hipStream_t stream) {
    SVPC_REQUIRE(n_cap >= 0 && lt >= 2, "seq_ul_fwd: caption rows of at least two positions");
    SVPC_REQUIRE(m >= 1 && m <= 64, "seq_ul_fwd: 1..64 negatives per position (one lane each)");
    if (n_cap > 0) {
        SVPC_REQUIRE(max_c >= 1 && max_c <= ld, "seq_ul_fwd: a row's columns must lie inside the score matrix");
        const long long waves = (long long)n_cap * (lt - 1);
        const long long blocks = (waves + kUlThreads / 64 - 1) / (kUlThreads / 64);
        SVPC_REQUIRE(blocks <= INT_MAX, "seq_ul_fwd: too many score rows for one launch");
        const dim3 grid((unsigned)blocks), block(kUlThreads);
        if (logits)
            hipLaunchKernelGGL(seq_ul_step_kernel<true>, grid, block, 0, stream, scores, ld, row_c, tgt, len, neg, m, n_cap, lt, unk, step,
                               ulstep);
        else
            hipLaunchKernelGGL(seq_ul_step_kernel<false>, grid, block, 0, stream, scores, ld, row_c, tgt, len, neg, m, n_cap, lt, unk, step,
                               ulstep);
        hipLaunchKernelGGL(seq_ul_finish_kernel, dim3((n_cap + 255) / 256), dim3(256), 0, stream, len, n_cap, lt, step, ulstep, cum, ul, barred);
    }
    hipLaunchKernelGGL(seq_ul_loss_kernel, dim3(1), dim3(256), 0, stream, cum, ul, barred, row_w, row_u, n_cap, loss);
    return svpc_check_launch("seq_ul_fwd");
}

int svpc_seq_ul_bwd(const float* scores, int ld, const int* row_c, int max_c, const int* tgt, const int* len, const int* barred,
                    const int* neg, int m, const float* row_w, const float* row_u, const float* dl, int n_cap, int lt, int logits, int unk,
                    float* dscores, int ld_out, hipStream_t stream) {
    if (n_cap == 0) return 0;
    SVPC_REQUIRE(n_cap > 0 && lt >= 2, "seq_ul_bwd: caption rows of at least two positions");
    SVPC_REQUIRE(m >= 1 && m <= 64, "seq_ul_bwd: 1..64 negatives per position (one lane each)");
    SVPC_REQUIRE(max_c >= 1 && max_c <= ld && ld_out >= 1, "seq_ul_bwd: a row's columns must lie inside the score matrix");
    const long long waves = (long long)n_cap * lt;
    const long long blocks = (waves + kUlThreads / 64 - 1) / (kUlThreads / 64);
    SVPC_REQUIRE(blocks <= INT_MAX, "seq_ul_bwd: too many score rows for one launch");
    const dim3 grid((unsigned)blocks), block(kUlThreads);
    if (logits)
        hipLaunchKernelGGL(seq_ul_bwd_kernel<true>, grid, block, 0, stream, scores, ld, row_c, tgt, len, barred, neg, m, row_w, row_u, dl,
                           n_cap, lt, unk, dscores, ld_out);
    else
        hipLaunchKernelGGL(seq_ul_bwd_kernel<false>, grid, block, 0, stream, scores, ld, row_c, tgt, len, barred, neg, m, row_w, row_u, dl,
                           n_cap, lt, unk, dscores, ld_out);
    return svpc_check_launch("seq_ul_bwd");
}

}  // extern "C"
