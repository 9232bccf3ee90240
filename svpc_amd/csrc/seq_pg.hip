// Clipped policy-gradient training over a video's K candidate paragraphs: PPO's clipped importance-ratio surrogate (Schulman
// et al. 2017) in its critic-free group form GRPO (Shao et al. 2024) with the per-token "k3" KL estimate against a frozen reference model;
// DAPO (Yu et al. 2025: clip-higher, token-level normalisation) and Dr. GRPO (Liu et al. 2025: no length normalisation) are settings of
// it.  The gradient coefficient differs at EVERY position — the ratio and the KL term are per token and the clip switches single tokens off
// — so the backward takes a weight per position where seq_nll.hip's takes one per caption.  Layout as seq_pref.hip: caption row r = t·K + k,
// the sentences of video b are the rows t = vid_off[b] … vid_off[b + 1] − 1, candidate paragraph k of a video is row k of each of its
// sentences.  Per candidate (b, k): n = max(1, Σ_t len[t, k]); valid: no sentence barred, adv[b, k] finite, every old_step / ref_step entry
// at its scored positions (i < len) finite.  In fp64 from the fp32 bits, per scored position (r, i) of a valid candidate:
//   s = step[r, i], o = old_step[r, i] (s itself without old_step), ρ = exp(s − o) (exactly 1 without old_step), A = adv[b, k];
//   sur = min(ρ·A, clamp(ρ, 1 − clip_lo, 1 + clip_hi)·A); under dual_clip = c > 1 and A < 0: sur = max(sur, c·A); A = 0: sur = 0;
//   active: sur is the unclipped ρ·A — not (A > 0 and ρ > 1 + clip_hi), not (A < 0 and ρ < 1 − clip_lo), not (A < 0 and ρ > c); strict;
//   δ = ref_step[r, i] − s, kl = exp(δ) − δ − 1 (0 without ref_step); tok = −sur + kl_beta·kl;
//   den = N·K·n (norm 0, "sequence"), max(1, n_tok) (1, "token": n_tok the scored positions of all valid candidates) or N·K (2, "none");
//   g = ∂tok / ∂s = −A·ρ·[active] + kl_beta·(1 − exp(δ));   pos_w[r, i] = fp32(row_w[r] − g / den), formed in fp64 and rounded once.
// On a candidate that is not valid the policy part is absent: pos_w[r, i] = row_w[r] at its scored positions; past a caption's end 0.
// loss = fp32(−Σ_{r not barred} row_w·cum + Σ tok / den), the second sum per row in position order, then over the rows in
// seq_nll_loss_kernel's order and tree; with no advantage of a valid candidate different from 0 and kl_beta = 0 it is not added at all.
// Restated by tests/pg_reference.py.
//
//   svpc_seq_pg_fwd       seven launches.  (1) … (3) svpc_seq_nll_fwd itself: step, cum and barred are its bits by construction (the loss
//                         it writes is overwritten by (7)).  (4) one wave per video, four per workgroup: all 64 lanes scan old_step /
//                         ref_step, one butterfly joins their masks, then lane k = candidate k: validity and n over the video's
//                         sentences, written per candidate (valid) and per caption row (row_adv = A or 0, row_n = n or 0).  (5) one
//                         workgroup: n_tok, thread t its rows
//                         t, t + 256, … then a fixed tree.  (6) one thread per caption row, over its positions in order: pos_w, pg, kl,
//                         n_clip, ratio_max and the row's Σ tok / den, EVERY element written.  (7) one workgroup: the loss.
//   svpc_seq_pos_bwd      seq_nll_bwd_kernel with the weight read per position and a per-row `dead` flag where it reads `barred`: one
//                         launch, EVERY element written; with pos_w[r, :] = row_w[r] and dead = barred its bits are svpc_seq_nll_bwd's.
//   svpc_group_advantage  one thread per video over its candidates with a finite reward, ascending k.
//
// No atomics; nothing allocates or synchronises; every launch is capturable.
#include "common.h"
#include "score_row.h"

#include <climits>

extern "C" int svpc_seq_nll_fwd(const float* scores, int ld, const int* row_c, int max_c, const int* tgt, const int* len, const float* row_w,
                                int n_cap, int lt, int logits, int unk, float* step, float* cum, int* barred, float* loss,
                                hipStream_t stream);

namespace {

constexpr int kPgThreads = 256;                // four videos (group kernel) / four score rows (backward) per workgroup
constexpr int kPgMaxK = 16;
enum { kPgSequence = 0, kPgToken = 1, kPgNone = 2 };
enum { kAdvGrpo = 0, kAdvCenter = 1, kAdvRloo = 2 };

__device__ __forceinline__ bool pg_candidate(int w, int C, int unk) { return w >= 0 && w < C && w != unk; }
__device__ __forceinline__ bool pg_finite(float v) { return v - v == 0.f; }
__device__ __forceinline__ bool pg_finite_d(double v) { return v - v == 0.0; }
__device__ __forceinline__ int pg_scored(int len, int steps) { return min(max(len, 0), steps); }

// One wave per video.  The scan of old_step / ref_step for a value that is not finite runs over all 64 lanes (element e of the video's
// contiguous rows × positions block goes to lane e mod 64: coalesced) and leaves a mask of candidates per lane; the masks are joined by a
// butterfly that EVERY lane executes (the only early return is wave-uniform; DESIGN 11.21's rule).  Then lane k = candidate k.
__global__ __launch_bounds__(kPgThreads) void seq_pg_group_kernel(const int* __restrict__ len, const int* __restrict__ barred,
                                                                  const double* __restrict__ adv, const float* __restrict__ old_step,
                                                                  const float* __restrict__ ref_step, const int* __restrict__ vid_off,
                                                                  int n_vid, int n_sent, int K, int lt, int* __restrict__ valid_out,
                                                                  double* __restrict__ row_adv, int* __restrict__ row_n) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * (kPgThreads / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (b >= n_vid) return;                       // (wave-uniform)
    // (wave-uniform) the video's sentences, clamped into the caption rows whatever the table holds
    const int t0 = min(max(vid_off[b], 0), n_sent);
    const int t1 = min(max(vid_off[b + 1], t0), n_sent);
    const int steps = lt - 1;
    int mask = 0;                                 // bit k: candidate k has an old_step / ref_step entry that is not finite where it is scored
    if (old_step != nullptr || ref_step != nullptr) {                       // (wave-uniform)
        const size_t r0 = (size_t)t0 * K;
        const int total = (t1 - t0) * K * steps;  // (n_sent·K·(lt − 1) fits an int: svpc_seq_pg_fwd)
        for (int e = lane; e < total; e += 64) {
            const int rr = e / steps, i = e - rr * steps;
            if (i >= pg_scored(len[r0 + rr], steps)) continue;
            bool ok = true;
            if (old_step != nullptr) ok = pg_finite(old_step[r0 * steps + e]);
            if (ref_step != nullptr) ok = ok && pg_finite(ref_step[r0 * steps + e]);
            if (!ok) mask |= 1 << (rr % K);
        }
        for (int o = 32; o > 0; o >>= 1) mask |= __shfl_xor(mask, o, 64);
    }
    if (lane >= K) return;
    long long words = 0;
    int bad = (mask >> lane) & 1;
    for (int t = t0; t < t1; ++t) {
        const size_t r = (size_t)t * K + lane;
        words += pg_scored(len[r], steps);
        bad |= barred[r];
    }
    const double A = adv[(size_t)b * K + lane];
    const bool valid = !bad && pg_finite_d(A);
    valid_out[(size_t)b * K + lane] = valid ? 1 : 0;
    const int n = (int)(words > 1 ? words : 1);
    for (int t = t0; t < t1; ++t) {
        const size_t r = (size_t)t * K + lane;
        row_adv[r] = valid ? A : 0.0;
        row_n[r] = valid ? n : 0;
    }
}

// n_tok: the scored positions of the valid candidates' caption rows
__global__ __launch_bounds__(256) void seq_pg_count_kernel(const int* __restrict__ len, const int* __restrict__ row_n, int n_cap, int lt,
                                                           int* __restrict__ n_tok) {
    __shared__ int part[256];
    int v = 0;
    for (int r = threadIdx.x; r < n_cap; r += 256)
        if (row_n[r] > 0) v += pg_scored(len[r], lt - 1);
    part[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) n_tok[0] = part[0];
}

__global__ __launch_bounds__(256) void seq_pg_row_kernel(const float* __restrict__ step, const float* __restrict__ old_step,
                                                         const float* __restrict__ ref_step, const int* __restrict__ len,
                                                         const float* __restrict__ row_w, const double* __restrict__ row_adv,
                                                         const int* __restrict__ row_n, const int* __restrict__ n_tok, int n_cap, int lt,
                                                         double groups, double lo, double hi, double dual, double kl_beta, int norm,
                                                         float* __restrict__ pos_w, double* __restrict__ pg, double* __restrict__ kl,
                                                         int* __restrict__ n_clip, float* __restrict__ ratio_max,
                                                         double* __restrict__ row_tok) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_cap) return;
    const int steps = lt - 1, n = pg_scored(len[r], steps), cand_n = row_n[r];
    const bool live = cand_n > 0;
    const double A = row_adv[r];
    const float w = row_w[r];
    double den = groups;                                                    // N·K
    if (norm == kPgSequence) den = groups * (double)(live ? cand_n : 1);
    if (norm == kPgToken) den = (double)max(n_tok[0], 1);
    double spg = 0.0, skl = 0.0, stok = 0.0, rmax = 0.0;
    int above = 0, below = 0;
    for (int i = 0; i < steps; ++i) {
        const size_t o = (size_t)r * steps + i;
        float out = 0.f;
        if (i < n) {
            out = w;
            if (live) {
                const double s = (double)step[o];
                const double rho = old_step != nullptr ? exp(s - (double)old_step[o]) : 1.0;
                const bool up = A > 0.0 && rho > 1.0 + hi;
                const bool deep = A < 0.0 && dual != 0.0 && rho > dual;
                const bool down = A < 0.0 && rho < 1.0 - lo;
                double sur = 0.0, g = 0.0;
                if (A != 0.0) {
                    sur = fmin(rho * A, fmin(fmax(rho, 1.0 - lo), 1.0 + hi) * A);
                    if (dual != 0.0 && A < 0.0) sur = fmax(sur, dual * A);
                    if (!up && !deep && !down) g = -(A * rho);
                }
                double k3 = 0.0;
                if (ref_step != nullptr) {
                    const double d = (double)ref_step[o] - s;
                    const double e = exp(d);
                    k3 = e - d - 1.0;
                    if (kl_beta != 0.0) g += kl_beta * (1.0 - e);
                }
                const double tok = kl_beta != 0.0 ? -sur + kl_beta * k3 : -sur;
                spg += -sur;
                skl += k3;
                stok += tok / den;
                above += (up || deep) ? 1 : 0;
                below += down ? 1 : 0;
                rmax = fmax(rmax, rho);
                out = (float)((double)w - g / den);
            }
        }
        pos_w[o] = out;
    }
    pg[r] = spg;
    kl[r] = skl;
    n_clip[2 * (size_t)r] = above;
    n_clip[2 * (size_t)r + 1] = below;
    ratio_max[r] = (float)rmax;
    row_tok[r] = stok;
}

// Σ of this thread's value over the workgroup in seq_nll_loss_kernel's tree, result in part[0]
__device__ __forceinline__ double pg_block_sum(double* part, double v) {
    __syncthreads();
    part[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    return part[0];
}

__global__ __launch_bounds__(256) void seq_pg_loss_kernel(const float* __restrict__ cum, const int* __restrict__ barred,
                                                          const float* __restrict__ row_w, const double* __restrict__ row_adv,
                                                          const double* __restrict__ row_tok, int n_cap, double kl_beta,
                                                          float* __restrict__ loss) {
    __shared__ double part[256];
    __shared__ int any;
    if (threadIdx.x == 0) any = kl_beta != 0.0 ? 1 : 0;
    __syncthreads();
    double v = 0.0, a = 0.0;
    int mine = 0;
    for (int r = threadIdx.x; r < n_cap; r += 256) {
        if (!barred[r]) v += (double)row_w[r] * (double)cum[r];
        a += row_tok[r];
        mine |= row_adv[r] != 0.0 ? 1 : 0;
    }
    if (mine) any = 1;                                                      // (every writer stores the same value)
    const double nll = pg_block_sum(part, v);
    const double tok = pg_block_sum(part, a);
    if (threadIdx.x == 0) {
        double out = -nll;
        if (any) out += tok;
        loss[0] = (float)out;
    }
}

template <bool LOGITS>
__global__ __launch_bounds__(kPgThreads) void seq_pos_bwd_kernel(const float* __restrict__ scores, int ld, const int* __restrict__ row_c,
                                                                 const int* __restrict__ tgt, const int* __restrict__ len,
                                                                 const int* __restrict__ dead, const float* __restrict__ pos_w,
                                                                 const float* __restrict__ dl, int n_cap, int lt, int unk,
                                                                 float* __restrict__ dscores, int ld_out) {
    const int lane = threadIdx.x & 63;
    const long long g = (long long)blockIdx.x * (kPgThreads / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (g >= (long long)n_cap * lt) return;       // (wave-uniform)
    const int r = (int)(g / lt), i = (int)(g - (long long)r * lt);
    float* out = dscores + (size_t)g * ld_out;
    const int C = row_c[r];
    const int w = i + 1 < lt ? tgt[(size_t)r * lt + i + 1] : -1;
    // (wave-uniform) a scored position of a caption that is not dead has a candidate target of finite step score
    if (i >= lt - 1 || i >= len[r] || dead[r] || !pg_candidate(w, C, unk)) {
        for (int c = lane; c < ld_out; c += 64) out[c] = 0.f;
        return;
    }
    const float* row = scores + (size_t)g * ld;
    const double s = (double)dl[0] * (double)pos_w[(size_t)r * (lt - 1) + i];
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

// one thread per video: the advantages of its candidates with a finite reward, ascending k; the others get 0
__global__ __launch_bounds__(256) void group_advantage_kernel(const double* __restrict__ reward, int n_vid, int K, int rule, double eps,
                                                              double* __restrict__ adv) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_vid) return;
    const double* r = reward + (size_t)b * K;
    double* a = adv + (size_t)b * K;
    int F = 0;
    double sum = 0.0, lo = 0.0, hi = 0.0;
    for (int k = 0; k < K; ++k) {
        const double v = r[k];
        if (!pg_finite_d(v)) continue;
        lo = F ? fmin(lo, v) : v;
        hi = F ? fmax(hi, v) : v;
        sum += v;
        ++F;
    }
    if (F < 2 || lo == hi) {                      // a test, not arithmetic: exactly 0
        for (int k = 0; k < K; ++k) a[k] = 0.0;
        return;
    }
    const double mean = sum / (double)F;
    double sd = 0.0;
    if (rule == kAdvGrpo) {
        double q = 0.0;
        for (int k = 0; k < K; ++k)
            if (pg_finite_d(r[k])) q += (r[k] - mean) * (r[k] - mean);
        sd = sqrt(q / (double)F);
    }
    for (int k = 0; k < K; ++k) {
        const double v = r[k];
        double out = 0.0;
        if (pg_finite_d(v)) {
            if (rule == kAdvRloo) {
                double others = 0.0;
                for (int j = 0; j < K; ++j)
                    if (j != k && pg_finite_d(r[j])) others += r[j];
                out = v - others / (double)(F - 1);
            } else if (rule == kAdvCenter) {
                out = v - mean;
            } else {
                out = (v - mean) / (sd + eps);
            }
        }
        a[k] = out;
    }
}

}  // namespace

extern "C" {

int svpc_seq_pg_fwd(const float* scores, int ld, const int* row_c, int max_c, const int* tgt, const int* len, const float* row_w,
                    const double* adv, const float* old_step, const float* ref_step, const int* vid_off, int n_vid, int n_sent, int k, int lt,
                    int logits, int unk, double clip_lo, double clip_hi, double dual_clip, double kl_beta, int norm, float* step, float* cum,
                    int* barred, float* pos_w, double* pg, double* kl, int* n_clip, float* ratio_max, int* valid, int* n_tok, double* row_adv,
                    int* row_n, double* row_tok, float* loss, hipStream_t stream) {
    SVPC_REQUIRE(n_vid >= 0 && n_sent >= 0 && lt >= 2, "seq_pg_fwd: caption rows of at least two positions");
    SVPC_REQUIRE(k >= 1 && k <= kPgMaxK, "seq_pg_fwd: 1..16 candidates per sentence (one lane each)");
    SVPC_REQUIRE((long long)n_sent * k * (lt - 1) <= INT_MAX, "seq_pg_fwd: too many scored positions");
    SVPC_REQUIRE(n_sent == 0 || n_vid >= 1, "seq_pg_fwd: caption rows belong to a video");
    SVPC_REQUIRE(clip_lo >= 0.0 && clip_lo < 1.0, "seq_pg_fwd: clip_lo lies in [0, 1)");
    SVPC_REQUIRE(clip_hi >= 0.0 && clip_hi - clip_hi == 0.0, "seq_pg_fwd: clip_hi is finite and not negative");
    SVPC_REQUIRE(dual_clip == 0.0 || (dual_clip > 1.0 && dual_clip - dual_clip == 0.0), "seq_pg_fwd: dual_clip is 0 (off) or finite and > 1");
    SVPC_REQUIRE(kl_beta >= 0.0 && kl_beta - kl_beta == 0.0, "seq_pg_fwd: kl_beta is finite and not negative");
    SVPC_REQUIRE(kl_beta == 0.0 || ref_step != nullptr, "seq_pg_fwd: kl_beta > 0 needs ref_step");
    SVPC_REQUIRE(norm >= kPgSequence && norm <= kPgNone, "seq_pg_fwd: norm 0 (sequence), 1 (token) or 2 (none)");
    const int n_cap = n_sent * k;
    // step, cum, barred: svpc_seq_nll_fwd's launches (its row checks too); the loss it writes is overwritten below
    const int rc = svpc_seq_nll_fwd(scores, ld, row_c, max_c, tgt, len, row_w, n_cap, lt, logits, unk, step, cum, barred, loss, stream);
    if (rc != 0) return rc;
    if (n_vid > 0) {
        const dim3 grid((unsigned)((n_vid + kPgThreads / 64 - 1) / (kPgThreads / 64))), block(kPgThreads);
        hipLaunchKernelGGL(seq_pg_group_kernel, grid, block, 0, stream, len, barred, adv, old_step, ref_step, vid_off, n_vid, n_sent, k, lt,
                           valid, row_adv, row_n);
    }
    hipLaunchKernelGGL(seq_pg_count_kernel, dim3(1), dim3(256), 0, stream, len, row_n, n_cap, lt, n_tok);
    if (n_cap > 0)
        hipLaunchKernelGGL(seq_pg_row_kernel, dim3((n_cap + 255) / 256), dim3(256), 0, stream, step, old_step, ref_step, len, row_w, row_adv,
                           row_n, n_tok, n_cap, lt, (double)n_vid * (double)k, clip_lo, clip_hi, dual_clip, kl_beta, norm, pos_w, pg, kl,
                           n_clip, ratio_max, row_tok);
    hipLaunchKernelGGL(seq_pg_loss_kernel, dim3(1), dim3(256), 0, stream, cum, barred, row_w, row_adv, row_tok, n_cap, kl_beta, loss);
    return svpc_check_launch("seq_pg_fwd");
}

int svpc_seq_pos_bwd(const float* scores, int ld, const int* row_c, int max_c, const int* tgt, const int* len, const int* dead,
                     const float* pos_w, const float* dl, int n_cap, int lt, int logits, int unk, float* dscores, int ld_out,
                     hipStream_t stream) {
    if (n_cap == 0) return 0;
    SVPC_REQUIRE(n_cap > 0 && lt >= 2, "seq_pos_bwd: caption rows of at least two positions");
    SVPC_REQUIRE(max_c >= 1 && max_c <= ld && ld_out >= 1, "seq_pos_bwd: a row's columns must lie inside the score matrix");
    const long long waves = (long long)n_cap * lt;
    const long long blocks = (waves + kPgThreads / 64 - 1) / (kPgThreads / 64);
    SVPC_REQUIRE(blocks <= INT_MAX, "seq_pos_bwd: too many score rows for one launch");
    const dim3 grid((unsigned)blocks), block(kPgThreads);
    if (logits)
        hipLaunchKernelGGL(seq_pos_bwd_kernel<true>, grid, block, 0, stream, scores, ld, row_c, tgt, len, dead, pos_w, dl, n_cap, lt, unk,
                           dscores, ld_out);
    else
        hipLaunchKernelGGL(seq_pos_bwd_kernel<false>, grid, block, 0, stream, scores, ld, row_c, tgt, len, dead, pos_w, dl, n_cap, lt, unk,
                           dscores, ld_out);
    return svpc_check_launch("seq_pos_bwd");
}

int svpc_group_advantage(const double* reward, int n_vid, int k, int rule, double eps, double* adv, hipStream_t stream) {
    SVPC_REQUIRE(n_vid >= 0 && k >= 1 && k <= kPgMaxK, "group_advantage: 1..16 candidates per video");
    SVPC_REQUIRE(rule >= kAdvGrpo && rule <= kAdvRloo, "group_advantage: rule 0 (grpo), 1 (center) or 2 (rloo)");
    SVPC_REQUIRE(eps >= 0.0 && eps - eps == 0.0, "group_advantage: eps is finite and not negative");
    if (n_vid == 0) return 0;
    hipLaunchKernelGGL(group_advantage_kernel, dim3((n_vid + 255) / 256), dim3(256), 0, stream, reward, n_vid, k, rule, eps, adv);
    return svpc_check_launch("group_advantage");
}

}  // extern "C"
