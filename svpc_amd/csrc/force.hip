// Forced decoding: the decoder's scores of captions it is handed (the GOLD score / gold perplexity of the reference's OpenNMT-derived
// translator lineage, next to the PRED score of its own decode).  The decoder side runs ONCE over all positions of all T·K caption rows
// (the all-positions pass of Translator._greedy_rerun: causal ∧ pad mask), so the score matrix has a row per (caption row r, step i):
// row r·Lt + i scores position p = i + 1 of caption r.  Three kernels (restated by tests/forced_score_reference.py):
//
//   svpc_force_inputs   per caption row: the walk over its extended ids y_1 … y_{Lt−1} — EOS at p ends it finished with len = p; PAD or
//                       IGNORE at p ends it unfinished with len = p − 1; otherwise len = Lt − 1 — the model-side ids (a copied word, or
//                       any id outside the text vocabulary, is UNK; PAD after position len), the fp32 text mask (1 on 0 … len) and the
//                       target column of every position (the id itself; what does not fit an int32 becomes −2, no column of any row).
//   svpc_force_score    one wave per score row (r, i) with i < len_r, several rows per workgroup, no LDS, no barrier: the lanes stride
//                       over the C_r columns once and collect the number of candidates (c < C_r, c ≠ UNK) ahead of the target w in the
//                       decoder's order (higher raw value, then lower column) and the best candidate; in logits mode the same pass takes
//                       the row maximum and a second pass (the row is 16 KB at most: it comes from the cache) the fp64 log-sum-exp
//                       without UNK, in beam.hip's order (score_row.h), so a step score here is the step score there.  A target that is
//                       no candidate (w = UNK, w < 0, w ≥ C_r) scores −inf (unk = "bar") or 0 (unk = "skip"), rank −1.  Rows past a
//                       caption's end return at once.
//   svpc_force_finish   one thread per caption row: cum = fp32(cum + step) in position order (the decoder's own accumulation), the
//                       positions that contributed (under "skip" a non-candidate does not), and the per-position outputs past the end
//                       set to (0, −1, −1, 0).
//
// Nothing allocates or synchronises; every launch is capturable.
#include "common.h"
#include "score_row.h"

#include <climits>

namespace {

constexpr int kForceThreads = 256;             // four score rows per workgroup

struct ForceScoreArgs {
    const float* scores; int ld; const int* row_c; const int* tgt; const int* len; int n_cap; int lt;
    int logits; int unk; int skip;
    float* step; int* rank; int* top; float* top_step;
};

template <typename IdT>
__global__ __launch_bounds__(256) void force_inputs_kernel(const IdT* __restrict__ ids, int n_cap, int lt,
                                                           int vocab, int unk, int eos, int pad, int ignore, int* __restrict__ model_ids,
                                                           float* __restrict__ mask, int* __restrict__ tgt, int* __restrict__ len,
                                                           int* __restrict__ finished) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_cap) return;
    const IdT* y = ids + (size_t)r * lt;
    int end = lt - 1, fin = 0;
    for (int p = 1; p < lt; ++p) {
        const long long w = (long long)y[p];
        if (w == eos) { end = p; fin = 1; break; }
        if (w == pad || w == ignore) { end = p - 1; break; }
    }
    for (int p = 0; p < lt; ++p) {
        const long long w = (long long)y[p];
        const size_t o = (size_t)r * lt + p;
        const bool in = p <= end;
        model_ids[o] = in ? ((w >= 0 && w < vocab) ? (int)w : unk) : pad;
        mask[o] = in ? 1.f : 0.f;
        tgt[o] = (w < -2 || w > INT_MAX) ? -2 : (int)w;
    }
    len[r] = end;
    finished[r] = fin;
}

__device__ __forceinline__ bool force_candidate(int w, int C, int unk) { return w >= 0 && w < C && w != unk; }

template <bool LOGITS>
__global__ __launch_bounds__(kForceThreads) void force_score_kernel(ForceScoreArgs a) {
    const int lane = threadIdx.x & 63;
    const long long g = (long long)blockIdx.x * (kForceThreads / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int steps = a.lt - 1;
    if (g >= (long long)a.n_cap * steps) return;  // (wave-uniform)
    const int r = (int)(g / steps), i = (int)(g - (long long)r * steps);
    if (i >= a.len[r]) return;                    // (wave-uniform) past the caption's end: svpc_force_finish writes the row
    const int C = a.row_c[r];
    const int w = a.tgt[(size_t)r * a.lt + i + 1];
    const bool cand = force_candidate(w, C, a.unk);
    const float* row = a.scores + ((size_t)r * a.lt + i) * a.ld;
    const float tv = cand ? row[w] : INFINITY;    // (no column is ahead of +inf at column −1: a non-candidate counts nothing)
    const int tw = cand ? w : -1;
    int ahead = 0;
    float bv = -INFINITY; int bc = INT_MAX;
    float m = -INFINITY;
    auto take = [&](float v, int c) {
        if (c == a.unk) return;
        ahead += raw_better(v, c, tv, tw) ? 1 : 0;
        if (raw_better(v, c, bv, bc)) { bv = v; bc = c; }
        if (LOGITS) m = fmaxf(m, v);
    };
    int c = lane;
    for (; c + 192 < C; c += 256) {               // four independent loads in flight per lane
        const float v0 = row[c], v1 = row[c + 64], v2 = row[c + 128], v3 = row[c + 192];
        take(v0, c); take(v1, c + 64); take(v2, c + 128); take(v3, c + 192);
    }
    for (; c < C; c += 64) take(row[c], c);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ahead += __shfl_xor(ahead, o, 64);
        const float ov = __shfl_xor(bv, o, 64); const int oc = __shfl_xor(bc, o, 64);
        if (raw_better(ov, oc, bv, bc)) { bv = ov; bc = oc; }
    }
    double lse = 0.0;
    if (LOGITS) lse = row_lse_from_max(row, C, a.unk, lane, m);
    if (lane == 0) {
        const size_t o = (size_t)r * steps + i;
        a.step[o] = cand ? step_score(tv, LOGITS ? 1 : 0, lse) : (a.skip ? 0.f : -INFINITY);
        a.rank[o] = cand ? ahead : -1;
        a.top[o] = bc == INT_MAX ? -1 : bc;
        a.top_step[o] = bc == INT_MAX ? -INFINITY : step_score(bv, LOGITS ? 1 : 0, lse);
    }
}

__global__ __launch_bounds__(256) void force_finish_kernel(const int* __restrict__ tgt, const int* __restrict__ len,
                                                           const int* __restrict__ row_c, int n_cap, int lt, int unk, int skip,
                                                           float* __restrict__ step, int* __restrict__ rank, int* __restrict__ top,
                                                           float* __restrict__ top_step, float* __restrict__ cum,
                                                           int* __restrict__ n_scored) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_cap) return;
    const int steps = lt - 1, n = len[r], C = row_c[r];
    float cu = 0.f;
    int ns = 0;
    for (int i = 0; i < steps; ++i) {
        const size_t o = (size_t)r * steps + i;
        if (i < n) {
            cu = cu + step[o];
            ns += (!skip || force_candidate(tgt[(size_t)r * lt + i + 1], C, unk)) ? 1 : 0;
        } else {
            step[o] = 0.f; rank[o] = -1; top[o] = -1; top_step[o] = 0.f;
        }
    }
    cum[r] = cu;
    n_scored[r] = ns;
}

// acc (9,) float64 += (captions, positions scored, Σ cum and Σ n_scored over the captions with a finite cum, captions with a non-finite
// cum, positions with rank 0, Σ rank and the count over the ranked positions, finished captions): one workgroup, every thread its rows
// r = tid, tid + 256, … in order, then a fixed tree over the threads — the same sums for the same input, run after run
constexpr int kForceAccCols = 9;

__global__ __launch_bounds__(256) void force_accum_kernel(const float* __restrict__ cum, const int* __restrict__ n_scored,
                                                          const int* __restrict__ finished, const int* __restrict__ len,
                                                          const int* __restrict__ rank, int n_cap, int lt, double* __restrict__ acc) {
    __shared__ double part[kForceAccCols][256];
    double v[kForceAccCols];
#pragma unroll
    for (int k = 0; k < kForceAccCols; ++k) v[k] = 0.0;
    const int steps = lt - 1;
    for (int r = threadIdx.x; r < n_cap; r += 256) {
        const float c = cum[r];
        const bool fin = c - c == 0.f;            // finite
        v[0] += 1.0;
        v[1] += (double)n_scored[r];
        if (fin) { v[2] += (double)c; v[3] += (double)n_scored[r]; } else v[4] += 1.0;
        const int n = min(len[r], steps);
        for (int i = 0; i < n; ++i) {
            const int k = rank[(size_t)r * steps + i];
            if (k >= 0) { v[5] += k == 0 ? 1.0 : 0.0; v[6] += (double)k; v[7] += 1.0; }
        }
        v[8] += finished[r] ? 1.0 : 0.0;
    }
#pragma unroll
    for (int k = 0; k < kForceAccCols; ++k) part[k][threadIdx.x] = v[k];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o)
            for (int k = 0; k < kForceAccCols; ++k) part[k][threadIdx.x] += part[k][threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x < kForceAccCols) acc[threadIdx.x] += part[threadIdx.x][0];
}

}  // namespace

extern "C" {

int svpc_force_inputs(const void* ids, int ids_i64, int n_cap, int lt, int vocab, int unk, int eos, int pad, int ignore,
                      int* model_ids, float* mask, int* tgt, int* len, int* finished, hipStream_t stream) {
    if (n_cap == 0) return 0;
    SVPC_REQUIRE(n_cap > 0 && lt >= 2, "force_inputs: caption rows of at least two positions");
    SVPC_REQUIRE(vocab > unk && unk >= 0, "force_inputs: the UNK id must lie inside the text vocabulary");
    const dim3 grid((n_cap + 255) / 256), block(256);
    if (ids_i64)
        hipLaunchKernelGGL(force_inputs_kernel<long long>, grid, block, 0, stream, (const long long*)ids, n_cap, lt, vocab, unk, eos,
                           pad, ignore, model_ids, mask, tgt, len, finished);
    else
        hipLaunchKernelGGL(force_inputs_kernel<int>, grid, block, 0, stream, (const int*)ids, n_cap, lt, vocab, unk, eos, pad, ignore,
                           model_ids, mask, tgt, len, finished);
    return svpc_check_launch("force_inputs");
}

int svpc_force_score(const float* scores, int ld, const int* row_c, int max_c, const int* tgt, const int* len, int n_cap, int lt, int logits,
                     int unk, int skip, float* step, int* rank, int* top, float* top_step, hipStream_t stream) {
    if (n_cap == 0) return 0;
    SVPC_REQUIRE(n_cap > 0 && lt >= 2, "force_score: caption rows of at least two positions");
    SVPC_REQUIRE(max_c >= 1 && max_c <= ld, "force_score: a row's columns must lie inside the score matrix");
    const long long waves = (long long)n_cap * (lt - 1);
    const long long blocks = (waves + kForceThreads / 64 - 1) / (kForceThreads / 64);
    SVPC_REQUIRE(blocks <= INT_MAX, "force_score: too many score rows for one launch");
    ForceScoreArgs a{scores, ld, row_c, tgt, len, n_cap, lt, logits, unk, skip, step, rank, top, top_step};
    const dim3 grid((unsigned)blocks), block(kForceThreads);
    if (logits) hipLaunchKernelGGL(force_score_kernel<true>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(force_score_kernel<false>, grid, block, 0, stream, a);
    return svpc_check_launch("force_score");
}

int svpc_force_finish(const int* tgt, const int* len, const int* row_c, int n_cap, int lt, int unk, int skip, float* step, int* rank,
                      int* top, float* top_step, float* cum, int* n_scored, hipStream_t stream) {
    if (n_cap == 0) return 0;
    SVPC_REQUIRE(n_cap > 0 && lt >= 2, "force_finish: caption rows of at least two positions");
    hipLaunchKernelGGL(force_finish_kernel, dim3((n_cap + 255) / 256), dim3(256), 0, stream, tgt, len, row_c, n_cap, lt, unk, skip, step, rank,
                       top, top_step, cum, n_scored);
    return svpc_check_launch("force_finish");
}

int svpc_force_accum(const float* cum, const int* n_scored, const int* finished, const int* len, const int* rank, int n_cap, int lt,
                     double* acc, hipStream_t stream) {
    if (n_cap == 0) return 0;
    SVPC_REQUIRE(n_cap > 0 && lt >= 2, "force_accum: caption rows of at least two positions");
    hipLaunchKernelGGL(force_accum_kernel, dim3(1), dim3(256), 0, stream, cum, n_scored, finished, len, rank, n_cap, lt, acc);
    return svpc_check_launch("force_accum");
}

}  // extern "C"
