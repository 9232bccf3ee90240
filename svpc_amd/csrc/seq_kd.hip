// Knowledge distillation against a teacher's per-position distribution (Hinton et al. 2015; Kim & Rush 2016, word level): on
// top of seq_nll.hip's −Σ w·log p(caption) the loss adds Σ v·kd, kd the sum over a caption's scored positions of the cross-entropy
// −Σ_c q_c·ℓ_c of the student's row against the teacher's row.  Layout as seq_nll.hip: n_cap caption rows of lt positions, score row
// r·lt + i scores position p = i + 1, i = 0 … lt − 2, scored while i < len[r].  Two fp32 matrices with the same rows, each with its own
// leading dimension and its own convention: the student `scores` (SL: raw logits, else probabilities) and the teacher `tq` (TL).  The
// candidates of a row are the columns c < C_r, c != unk.  In fp64:
//   q_c   teacher probability: raw > 0 ? raw : 0, or exp(raw − lse_q), lse_q the teacher row's log-sum-exp without unk in beam.hip's order
//         (a row whose lse_q is not finite — no finite candidate logit — has q = 0 everywhere); never renormalised; 0 at unk;
//   ℓ_c   student log-probability: log p_c, or raw − lse with no exp / log round trip;
//   a column with q_c > 0 is CLAMPED when p_c <= 0 or ℓ_c < log ε, ε = 2^-100 (for an fp32 probability: p_c < ε, an exact comparison): its
//         term is −q_c·log ε and its gradient zero.
// Restated by tests/distill_reference.py.
//
//   svpc_seq_kd_fwd     three launches as svpc_seq_nll_fwd.  (1) one wave per score row (r, i), i < len[r], four per workgroup: the target's
//                       step score through score_row.h (seq_nll.hip's bits), then ONE pass over both rows: per lane the columns lane,
//                       lane + 64, … ascending, kdstep = fp32(−Σ q_c·ℓ_c) and hstep = fp32(−Σ q_c·log q_c) over the candidates with
//                       q_c > 0 (the logs are skipped where q_c = 0), the lanes joined by the fixed butterfly; rows past the end return
//                       before any column work.  (2) one thread per caption: cum, barred, kd = fp32(kd + kdstep), ent = fp32(ent + hstep)
//                       in position order, zeroes past the end.  (3) one workgroup: loss = fp32(−Σ w_r·cum_r + Σ v_r·kd_r) over the
//                       captions that are not barred, seq_nll_loss_kernel's order; a caption with v_r = 0 adds seq_nll's term alone.
//   svpc_seq_kd_bwd     one wave per row of the (n_cap·lt, ld_out) gradient, EVERY element written once by the lane that owns its column:
//                       the zero rows and columns of svpc_seq_nll_bwd; else, probabilities, −dl·(w·[c = y] / p_y + v·q_c / p_c), the second
//                       term for unclamped columns with q_c > 0; logits, dl·[w·(p_c − [c = y]) + v·(Q′·p_c − q′_c)], q′ = q on the unclamped
//                       columns, Q′ = Σ q′, 0 at unk.  lse, lse_q and Q′ are taken by re-reading the rows (as seq_nll_bwd_kernel<true>
//                       re-reads its row); no side buffer.  A row with dl·v = 0 is seq_nll_bwd_kernel's row, bit for bit.
//
// Nothing allocates or synchronises; every launch is capturable.
#include "common.h"
#include "score_row.h"

#include <climits>

namespace {

constexpr int kKdThreads = 256;                                      // four score rows per workgroup
constexpr double kKdLogEps = -100.0 * 0.6931471805599453094;         // log ε, ε = 2^-100: a defined constant, not a tolerance
constexpr double kKdEps = 0x1p-100;                                  // ε, exact in fp32 and fp64

__device__ __forceinline__ bool kd_candidate(int w, int C, int unk) { return w >= 0 && w < C && w != unk; }
__device__ __forceinline__ bool kd_finite(float v) { return v - v == 0.f; }
__device__ __forceinline__ bool kd_finite_d(double v) { return v - v == 0.0; }

// the teacher's probability of a candidate column with raw value v
template <bool TL>
__device__ __forceinline__ double kd_q(float v, double lse_q, bool q_ok) {
    if (TL) return q_ok ? exp((double)v - lse_q) : 0.0;
    return v > 0.f ? (double)v : 0.0;
}

// the student's side of a column with q > 0: its log-probability, and whether the clamp holds it
template <bool SL>
__device__ __forceinline__ bool kd_student(float v, double lse, double* l) {
    if (SL) {
        *l = (double)v - lse;
        return *l < kKdLogEps;
    }
    const double p = (double)v;
    if (p <= 0.0 || p < kKdEps) return true;
    *l = log(p);
    return false;
}

template <bool SL, bool TL>
__global__ __launch_bounds__(kKdThreads) void seq_kd_step_kernel(const float* __restrict__ scores, int ld, const float* __restrict__ tq,
                                                                 int ldq, const int* __restrict__ row_c, int max_c,
                                                                 const int* __restrict__ tgt, const int* __restrict__ len, int n_cap,
                                                                 int lt, int unk, float* __restrict__ step, float* __restrict__ kdstep,
                                                                 float* __restrict__ hstep) {
    const int lane = threadIdx.x & 63;
    const long long g = (long long)blockIdx.x * (kKdThreads / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int steps = lt - 1;
    if (g >= (long long)n_cap * steps) return;    // (wave-uniform)
    const int r = (int)(g / steps), i = (int)(g - (long long)r * steps);
    if (i >= len[r]) return;                      // (wave-uniform) past the caption's end: the finish kernel writes the entries
    const int C = min(row_c[r], max_c);           // (a column count past the matrices reads nothing outside them)
    const int w = tgt[(size_t)r * lt + i + 1];
    const float* row = scores + ((size_t)r * lt + i) * ld;
    const float* trow = tq + ((size_t)r * lt + i) * ldq;
    double lse = 0.0, lse_q = 0.0;
    if (SL) lse = row_lse(row, C, unk, lane);
    if (TL) lse_q = row_lse(trow, C, unk, lane);
    const bool q_ok = !TL || kd_finite_d(lse_q);  // (wave-uniform)
    float s = -INFINITY;
    if (kd_candidate(w, C, unk)) s = step_score(row[w], SL ? 1 : 0, lse);      // (wave-uniform)
    double akd = 0.0, ah = 0.0;
    for (int c = lane; c < C; c += 64) {
        if (c == unk) continue;
        const float tv = trow[c], sv = row[c];
        const double q = kd_q<TL>(tv, lse_q, q_ok);
        if (q > 0.0) {
            double l = 0.0;
            const bool clamped = kd_student<SL>(sv, lse, &l);
            akd -= q * (clamped ? kKdLogEps : l);
            ah -= q * (TL ? (double)tv - lse_q : log(q));
        }
    }
    akd = wave_sum_d(akd);
    ah = wave_sum_d(ah);
    if (lane == 0) {
        step[g] = s;
        kdstep[g] = (float)akd;
        hstep[g] = (float)ah;
    }
}

__global__ __launch_bounds__(256) void seq_kd_finish_kernel(const int* __restrict__ len, int n_cap, int lt, float* __restrict__ step,
                                                            float* __restrict__ kdstep, float* __restrict__ hstep, float* __restrict__ cum,
                                                            float* __restrict__ kd, float* __restrict__ ent, int* __restrict__ barred) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_cap) return;
    const int steps = lt - 1, n = len[r];
    float cu = 0.f, ku = 0.f, hu = 0.f;
    int bar = 0;
    for (int i = 0; i < steps; ++i) {
        const size_t o = (size_t)r * steps + i;
        if (i < n) {
            const float s = step[o];
            cu = cu + s;
            ku = ku + kdstep[o];
            hu = hu + hstep[o];
            bar |= kd_finite(s) ? 0 : 1;
        } else {
            step[o] = 0.f;
            kdstep[o] = 0.f;
            hstep[o] = 0.f;
        }
    }
    cum[r] = cu;
    kd[r] = ku;
    ent[r] = hu;
    barred[r] = bar;
}

__global__ __launch_bounds__(256) void seq_kd_loss_kernel(const float* __restrict__ cum, const float* __restrict__ kd,
                                                          const int* __restrict__ barred, const float* __restrict__ row_w,
                                                          const float* __restrict__ row_v, int n_cap, float* __restrict__ loss) {
    __shared__ double part[256];
    double v = 0.0;
    for (int r = threadIdx.x; r < n_cap; r += 256)
        if (!barred[r]) {
            v += (double)row_w[r] * (double)cum[r];
            const double vr = (double)row_v[r];
            if (vr != 0.0) v -= vr * (double)kd[r];
        }
    part[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = (float)(-part[0]);
}

template <bool SL, bool TL>
__global__ __launch_bounds__(kKdThreads) void seq_kd_bwd_kernel(const float* __restrict__ scores, int ld, const float* __restrict__ tq,
                                                                int ldq, const int* __restrict__ row_c, int max_c,
                                                                const int* __restrict__ tgt, const int* __restrict__ len,
                                                                const int* __restrict__ barred, const float* __restrict__ row_w,
                                                                const float* __restrict__ row_v, const float* __restrict__ dl, int n_cap,
                                                                int lt, int unk, float* __restrict__ dscores, int ld_out) {
    const int lane = threadIdx.x & 63;
    const long long g = (long long)blockIdx.x * (kKdThreads / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (g >= (long long)n_cap * lt) return;       // (wave-uniform)
    const int r = (int)(g / lt), i = (int)(g - (long long)r * lt);
    float* out = dscores + (size_t)g * ld_out;
    const int C = min(row_c[r], max_c);
    const int w = i + 1 < lt ? tgt[(size_t)r * lt + i + 1] : -1;
    // (wave-uniform) a scored position of a caption that is not barred has a candidate target of finite step score
    if (i >= lt - 1 || i >= len[r] || barred[r] || !kd_candidate(w, C, unk)) {
        for (int c = lane; c < ld_out; c += 64) out[c] = 0.f;
        return;
    }
    const float* row = scores + (size_t)g * ld;
    const float* trow = tq + (size_t)g * ldq;
    const double s = (double)dl[0] * (double)row_w[r];
    const double sv = (double)dl[0] * (double)row_v[r];
    const bool with_v = sv != 0.0;                // (wave-uniform) without it the row is seq_nll_bwd_kernel's, bit for bit
    double lse_q = 0.0;
    bool q_ok = true;
    if (TL && with_v) {                           // (wave-uniform)
        lse_q = row_lse(trow, C, unk, lane);
        q_ok = kd_finite_d(lse_q);
    }
    if (SL) {
        const double lse = row_lse(row, C, unk, lane);
        double Qp = 0.0;
        if (with_v) {                             // (wave-uniform) Q′: the teacher's mass on the unclamped columns
            for (int c = lane; c < C; c += 64) {
                if (c == unk) continue;
                const double q = kd_q<TL>(trow[c], lse_q, q_ok);
                if (q > 0.0 && !((double)row[c] - lse < kKdLogEps)) Qp += q;
            }
            Qp = wave_sum_d(Qp);
        }
        for (int c = lane; c < ld_out; c += 64) {
            float d = 0.f;
            if (c < C && c != unk) {
                const double l = (double)row[c] - lse;
                const double p = exp(l);
                double v = s * (p - (c == w ? 1.0 : 0.0));
                if (with_v) {
                    const double q = kd_q<TL>(trow[c], lse_q, q_ok);
                    v += sv * (Qp * p - ((q > 0.0 && !(l < kKdLogEps)) ? q : 0.0));
                }
                d = (float)v;
            }
            out[c] = d;
        }
    } else {
        const double dw = -s / (double)row[w];
        if (!with_v) {                            // (wave-uniform)
            const float d = (float)dw;
            for (int c = lane; c < ld_out; c += 64) out[c] = c == w ? d : 0.f;
            return;
        }
        for (int c = lane; c < ld_out; c += 64) {
            float d = c == w ? (float)dw : 0.f;
            if (c < C && c != unk) {
                const double q = kd_q<TL>(trow[c], lse_q, q_ok);
                const double p = (double)row[c];
                if (q > 0.0 && !(p <= 0.0 || p < kKdEps)) d = (float)((c == w ? dw : 0.0) - sv * q / p);
            }
            out[c] = d;
        }
    }
}

}  // namespace

extern "C" {

int svpc_seq_kd_fwd(const float* scores, int ld, const float* tq, int ldq, const int* row_c, int max_c, const int* tgt, const int* len,
                    const float* row_w, const float* row_v, int n_cap, int lt, int logits, int teacher_logits, int unk, float* step,
                    float* kdstep, float* hstep, float* cum, float* kd, float* ent, int* barred, float* loss, hipStream_t stream) {
    SVPC_REQUIRE(n_cap >= 0 && lt >= 2, "seq_kd_fwd: caption rows of at least two positions");
    if (n_cap > 0) {
        SVPC_REQUIRE(max_c >= 1 && max_c <= ld && max_c <= ldq, "seq_kd_fwd: a row's columns must lie inside the student's and the teacher's matrix");
        const long long waves = (long long)n_cap * (lt - 1);
        const long long blocks = (waves + kKdThreads / 64 - 1) / (kKdThreads / 64);
        SVPC_REQUIRE(blocks <= INT_MAX, "seq_kd_fwd: too many score rows for one launch");
        const dim3 grid((unsigned)blocks), block(kKdThreads);
#define SVPC_KD_STEP(SL, TL)                                                                                                              \
    hipLaunchKernelGGL((seq_kd_step_kernel<SL, TL>), grid, block, 0, stream, scores, ld, tq, ldq, row_c, max_c, tgt, len, n_cap, lt, unk, \
                       step, kdstep, hstep)
        if (logits && teacher_logits) SVPC_KD_STEP(true, true);
        else if (logits) SVPC_KD_STEP(true, false);
        else if (teacher_logits) SVPC_KD_STEP(false, true);
        else SVPC_KD_STEP(false, false);
#undef SVPC_KD_STEP
        hipLaunchKernelGGL(seq_kd_finish_kernel, dim3((n_cap + 255) / 256), dim3(256), 0, stream, len, n_cap, lt, step, kdstep, hstep, cum, kd,
                           ent, barred);
    }
    hipLaunchKernelGGL(seq_kd_loss_kernel, dim3(1), dim3(256), 0, stream, cum, kd, barred, row_w, row_v, n_cap, loss);
    return svpc_check_launch("seq_kd_fwd");
}

int svpc_seq_kd_bwd(const float* scores, int ld, const float* tq, int ldq, const int* row_c, int max_c, const int* tgt, const int* len,
                    const int* barred, const float* row_w, const float* row_v, const float* dl, int n_cap, int lt, int logits,
                    int teacher_logits, int unk, float* dscores, int ld_out, hipStream_t stream) {
    if (n_cap == 0) return 0;
    SVPC_REQUIRE(n_cap > 0 && lt >= 2, "seq_kd_bwd: caption rows of at least two positions");
    SVPC_REQUIRE(max_c >= 1 && max_c <= ld && max_c <= ldq && ld_out >= 1,
                 "seq_kd_bwd: a row's columns must lie inside the student's and the teacher's matrix");
    const long long waves = (long long)n_cap * lt;
    const long long blocks = (waves + kKdThreads / 64 - 1) / (kKdThreads / 64);
    SVPC_REQUIRE(blocks <= INT_MAX, "seq_kd_bwd: too many score rows for one launch");
    const dim3 grid((unsigned)blocks), block(kKdThreads);
#define SVPC_KD_BWD(SL, TL)                                                                                                               \
    hipLaunchKernelGGL((seq_kd_bwd_kernel<SL, TL>), grid, block, 0, stream, scores, ld, tq, ldq, row_c, max_c, tgt, len, barred, row_w,   \
                       row_v, dl, n_cap, lt, unk, dscores, ld_out)
    if (logits && teacher_logits) SVPC_KD_BWD(true, true);
    else if (logits) SVPC_KD_BWD(true, false);
    else if (teacher_logits) SVPC_KD_BWD(false, true);
    else SVPC_KD_BWD(false, false);
#undef SVPC_KD_BWD
    return svpc_check_launch("seq_kd_bwd");
}

}  // extern "C"
