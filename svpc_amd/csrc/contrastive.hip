// Contrastive search (Su et al. 2022, "A Contrastive Framework for Neural Text Generation"; HuggingFace generate(penalty_alpha, top_k)): one
// selection step over the k candidate rows of every sentence.  The decoder side, the ping-pong id and ancestry tables, the launch shape and
// the row scan are the beam decode's (beam_common.h); the state is per SENTENCE — one committed caption, its summed step score, its length,
// and the last-layer hidden state of every committed position (the history) — and per row only the candidate the row carries.
//
// Iteration i = pos runs AFTER the decoder pass over the k rows at position i, whose row r carries one candidate word for position i (its
// extended id is ext_in[r][i]) with p_r (cand_p, the model's probability of the word; 0: a dead candidate, which can never win) and s_r
// (cand_score, score_row.h's step score of the word in its parent's row).  hidden[r] is the pass's last-layer output of row r, h_r.  Restated
// by tests/contrastive_reference.py::select:
//   penalty_r = max_{j < i} cos(h_r, H[t, j])   (0 at i = 0: no history),  cos = dot / (sqrt(|h_r|²)·sqrt(|H_j|²)), 0 when a norm is 0;
//   score_r   = (1 − α)·p_r − α·penalty_r       (fp64);  the winner: the highest score among the live rows, ties to the lowest row;
//   commit:     ids[t, i] = the winner's extended id, cum[t] += s_winner (fp32), len[t] = i, pen[t, i] = penalty_winner, H[t, i] = h_winner
//               with its squared norm beside it; EOS finishes the sentence;
//   expansion   (i + 1 < Lt, the sentence not finished): the top k columns of the winner's score row by (higher raw value, lower column),
//               without UNK, without EOS while i + 1 ≤ min_len, become the k rows' candidates at position i + 1: p the raw value (≤ 0: 0), in
//               logits mode fp32(exp(raw − lse)); s the step score; a column with p = 0, or a missing one, is dead: PAD, p 0, s −inf.  Every
//               child takes the winner's token rows and ancestry for positions ≤ i and its own slot at i + 1.
// A finished sentence writes PAD children and changes nothing else; a sentence without a live candidate finishes with PAD and cum = −inf.
// At i = 0 the host starts row 0 alone live (p 1, s 0) on BOS, so it wins and its hidden state becomes history entry 0.
//
// One 256-thread workgroup per sentence.  Dot products and squared norms of the fp32 hidden states are summed in fp64 — per lane the
// elements lane, lane + 64, … in that order, then wave_sum_d's butterfly: a fixed order, so the stored norms are reproducible bit for bit.
//   phase 1: the k·i (candidate, history entry) pairs dealt to the four waves — a wave owns one candidate (k > 4: two) and, for k ≤ 2,
//            a share of the history entries —, one dot product over D per pair, eight entries at a time so that their loads and
//            butterflies overlap (a short batch repeats its last entry); a wave takes its candidate's squared norm first and keeps the running maximum cosine  → LDS
//   phase 2: one lane ranks the ≤ 8 scores and publishes the winner
//   phase 3: wave 0 scans the winner's score row (topb_row, row_lse in logits mode) while waves 1 … 3 copy h_winner into the history and
//            commit; after a barrier the children are stored and the winner's token and ancestry rows copied (copy_parent_rows).
// Everything of the parents that a later phase reads (cand_p, cand_score, the candidates' ids, cum, finished) is loaded before any write; no
// atomics; every branch around a cross-lane step is wave-uniform (the sentence's state and the winner are workgroup-uniform).
#include "beam_common.h"

namespace {

constexpr int kContrastiveCols = 4096;             // columns of a score row (ops.SAMPLE_COLS_MAX)
constexpr int kWaves = kBeamThreads / 64;

struct ContrastiveArgs {
    const float* hidden; int ld_h; int D; double alpha; int min_len; int max_c;
    float* cand_p; float* cand_score;
    int* ids; float* pen; int* len; float* hist; double* hist_n2; int* winner;
};

// Σ_d x[d]·y[d] over D in fp64 by the 64 lanes of a wave, every lane returns with the sum (the product of two fp32 is exact in fp64)
__device__ __forceinline__ double wave_dot_d(const float* x, const float* y, int D, int lane) {
    double s = 0.0;
    for (int d = lane; d < D; d += 64) s += (double)x[d] * (double)y[d];
    return wave_sum_d(s);
}

// the same for N rows y[0 … N) at once → s[0 … N): each sum in wave_dot_d's order, the N chains of loads and shuffles independent
constexpr int kDotRows = 8;
template <int N>
__device__ __forceinline__ void wave_dotn_d(const float* x, const float* const (&y)[N], int D, int lane, double (&s)[N]) {
#pragma unroll
    for (int q = 0; q < N; ++q) s[q] = 0.0;
    for (int d = lane; d < D; d += 64) {
        const double xv = (double)x[d];
#pragma unroll
        for (int q = 0; q < N; ++q) s[q] += xv * (double)y[q][d];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int q = 0; q < N; ++q) s[q] += __shfl_xor(s[q], o, 64);
    }
}

// cos of a pair from its dot product, |h|² = nr with sr = sqrt(nr), and |H_j|² = nj: 0 when either norm is 0
__device__ __forceinline__ double cosine_d(double dot, double nr, double sr, double nj) {
    return (nr > 0.0 && nj > 0.0) ? dot / (sr * sqrt(nj)) : 0.0;
}

// In this kernel BeamArgs::cum and BeamArgs::finished are per SENTENCE ((n_sent,), not per row).
template <int B>
__global__ __launch_bounds__(kBeamThreads) void contrastive_step_kernel(BeamArgs a, ContrastiveArgs ca) {
    __shared__ double c_n2[B];                     // the candidates' squared norms
    constexpr int G = B <= kWaves ? kWaves / B : 1;      // the waves that share one candidate's history entries
    __shared__ double w_pen[G][B];                 // per group: the largest cosine it saw of every candidate
    __shared__ float c_p[B], c_s[B];               // the candidates' p and step score
    __shared__ int c_ext[B];                       // … and extended ids
    __shared__ double s_pen;                       // the winner's penalty
    __shared__ int s_win;                          // the winner (−1: none)
    __shared__ float n_p[B], n_s[B];               // the children's p and step score
    __shared__ int n_col[B];                       // … and columns (−1: dead)
    __shared__ int sel[B];
    const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r0 = t * B, i = a.pos, pl = a.pos + 1, Lt = a.ld_tok, D = ca.D;
    const bool was_fin = a.finished[t] != 0;       // (workgroup-uniform)
    const float cum0 = a.cum[t];
    const float* hist = ca.hist + (size_t)t * Lt * D;
    const double* hist_n2 = ca.hist_n2 + (size_t)t * Lt;
    if (tid < B) {
        c_p[tid] = ca.cand_p[r0 + tid];
        c_s[tid] = ca.cand_score[r0 + tid];
        c_ext[tid] = a.ext_in[(size_t)(r0 + tid) * Lt + i];
    }
    // ---- phases 0 and 1: the B·i (candidate, history entry) pairs dealt to the four waves.  B <= 4: wave w takes candidate w % B and the
    // entries g, g + G, … of group g = w / B, G = 4 / B groups (B = 3: the fourth wave idles); B > 4: candidates w and w + 4, every entry.
    // A wave first takes its candidate's squared norm, then kDotRows entries at a time: their loads and butterflies are independent chains.
    if (!was_fin) {
        const int g = B <= kWaves ? wave / B : 0;
        for (int r = B <= kWaves ? wave % B : wave; r < B && g < G; r += kWaves) {      // (wave-uniform)
            const float* h = ca.hidden + (size_t)(r0 + r) * ca.ld_h;
            const double nr = wave_dot_d(h, h, D, lane);
            if (lane == 0 && g == 0) c_n2[r] = nr;
            const double sr = sqrt(nr);
            double mx = -INFINITY;
            const int j_last = i > g ? g + (i - 1 - g) / G * G : g;      // the group's last entry; a short batch repeats it (the maximum is the same)
            for (int j = g; j < i; j += kDotRows * G) {
                const float* y[kDotRows]; int jq[kDotRows]; double s[kDotRows];
#pragma unroll
                for (int q = 0; q < kDotRows; ++q) { jq[q] = min(j + q * G, j_last); y[q] = hist + (size_t)jq[q] * D; }
                wave_dotn_d<kDotRows>(h, y, D, lane, s);
#pragma unroll
                for (int q = 0; q < kDotRows; ++q) mx = fmax(mx, cosine_d(s[q], nr, sr, hist_n2[jq[q]]));
            }
            if (lane == 0) w_pen[g][r] = mx;
        }
    }
    __syncthreads();
    // ---- phase 2: one lane ranks the live candidates by strict comparison from row 0 up (ties to the lowest row)
    if (tid == 0) {
        int w = -1; double best = 0.0, bpen = 0.0;
        if (!was_fin) {
            for (int r = 0; r < B; ++r) {
                if (!(c_p[r] > 0.f)) continue;
                double pn = 0.0;
                if (i > 0) {
                    pn = w_pen[0][r];
                    for (int q = 1; q < G; ++q) pn = fmax(pn, w_pen[q][r]);
                }
                const double sc = (1.0 - ca.alpha) * (double)c_p[r] - ca.alpha * pn;
                if (w < 0 || sc > best) { w = r; best = sc; bpen = pn; }
            }
        }
        s_win = w; s_pen = bpen;
    }
    __syncthreads();
    // ---- phase 3
    const int w = s_win;                          // (workgroup-uniform)
    const bool live = w >= 0;
    const int par = r0 + (live ? w : 0);          // the row the children descend from (a finished sentence: row 0, whose rows are valid)
    const bool ends = !live || c_ext[live ? w : 0] == a.eos;     // no child is a candidate: finished before, finishing now, or nothing live
    const bool expand = pl < Lt;
    if (wave == 0) {
        float v = -INFINITY; int c = INT_MAX; double lse = 0.0;
        if (expand && !ends) {                    // (wave-uniform) the winner's row: its top B columns under the EOS filter
            const int C = max(min(a.row_c[par], ca.max_c), 0);
            const float* row = a.scores + (size_t)par * a.ld;
            lse = a.logits ? row_lse(row, C, a.unk, lane) : 0.0;
            const int skip_eos = pl <= ca.min_len ? a.eos : a.unk;
            float val[B]; int idx[B];
            topb_row<B>(val, idx, C, lane, a.unk, skip_eos, RawKey{row}, NoBan{});
            topb_entry<B>(val, idx, lane, v, c);
        }
        if (lane < B) {
            float p = 0.f;
            if (c != INT_MAX) p = a.logits ? (float)exp((double)v - lse) : (v > 0.f ? v : 0.f);
            const bool dead = !(p > 0.f);
            n_p[lane] = dead ? 0.f : p;
            n_s[lane] = dead ? -INFINITY : step_score(v, a.logits, lse);
            n_col[lane] = dead ? -1 : c;
            sel[lane] = par - r0;
        }
    } else if (!was_fin) {                        // (wave-uniform) the commit
        if (live) {
            const float* h = ca.hidden + (size_t)(r0 + w) * ca.ld_h;
            float* dst = ca.hist + ((size_t)t * Lt + i) * D;
            for (int d = tid - 64; d < D; d += kBeamThreads - 64) dst[d] = h[d];
        }
        if (tid == 64) {
            const size_t o = (size_t)t * Lt + i;
            if (live) {
                ca.hist_n2[o] = c_n2[w];
                ca.ids[o] = c_ext[w];
                ca.pen[o] = (float)s_pen;
                ca.len[t] = i;
                a.cum[t] = cum0 + c_s[w];
                a.finished[t] = c_ext[w] == a.eos ? 1 : 0;
            } else {                              // no live candidate: the sentence ends dead
                ca.ids[o] = a.pad;
                a.cum[t] = -INFINITY;
                a.finished[t] = 1;
            }
        }
    }
    if (tid == 64) ca.winner[t] = w;
    if (!expand) return;                          // (workgroup-uniform) the last position has no children
    __syncthreads();
    if (tid < B) {                                // child tid: the winner's column n_col[tid] at position pl, or PAD
        const int r = r0 + tid, col = n_col[tid];
        const int C = max(min(a.row_c[par], ca.max_c), 0), X = a.row_x[par];
        const int ext = col < 0 ? a.pad : col;
        const int mod = col < 0 ? a.pad : (col >= C - X ? a.unk : col);
        ca.cand_p[r] = n_p[tid];
        ca.cand_score[r] = n_s[tid];
        a.parent[r] = par;
        a.next_ext[r] = ext;
        a.next_model[r] = mod;
        a.text_out[(size_t)r * Lt + pl] = mod;
        a.ext_out[(size_t)r * Lt + pl] = ext;
        a.rows_out[(size_t)r * Lt + pl] = r * a.slot_rows + pl;
    }
    copy_parent_rows<B>(a, r0, pl, tid, sel);
}

}  // namespace

extern "C" int svpc_contrastive_step(const float* scores, int ld, const int* row_c, const int* row_x, int n_sent, int k, int pos, int logits,
                                     int unk, int eos, int pad, int slot_rows, const float* hidden, int ld_h, int d, double alpha, int min_len,
                                     int max_c, float* cand_p, float* cand_score, const int* text_in, const int* ext_in, const int* rows_in,
                                     int* text_out, int* ext_out, int* rows_out, int ld_tok, int* parent, int* next_ext, int* next_model,
                                     int* ids, float* cum, int* len, float* pen, int* finished, float* hist, double* hist_n2, int* winner,
                                     hipStream_t stream) {
    if (n_sent == 0) return 0;
    SVPC_REQUIRE(k >= 1 && k <= kBeamMax, "contrastive_step: top_k must be 1..8");
    SVPC_REQUIRE(d >= 1 && ld_h >= d, "contrastive_step: the hidden size must be >= 1 and within the hidden rows");
    SVPC_REQUIRE(pos >= 0 && pos < ld_tok, "contrastive_step: position pos must lie inside the token / ancestry rows (0 <= pos < Lt)");
    SVPC_REQUIRE(slot_rows >= ld_tok, "contrastive_step: a cache slot holds at least Lt rows");
    SVPC_REQUIRE(max_c >= 1 && max_c <= kContrastiveCols && (scores == nullptr || max_c <= ld),
                 "contrastive_step: row columns must be 1..4096 and within ld");
    SVPC_REQUIRE(scores != nullptr || pos + 1 == ld_tok, "contrastive_step: only the last position runs without score rows");
    SVPC_REQUIRE(alpha >= 0.0 && alpha <= 1.0, "contrastive_step: penalty_alpha must be a finite number in [0, 1]");
    SVPC_REQUIRE(min_len >= 0 && min_len < ld_tok, "contrastive_step: min length must be 0..ld_tok-1");
    SVPC_REQUIRE(text_in != text_out && ext_in != ext_out && rows_in != rows_out, "contrastive_step: the token and ancestry tables are ping-pong pairs");
    SVPC_REQUIRE(hidden != nullptr && cand_p != nullptr && cand_score != nullptr && ids != nullptr && cum != nullptr && len != nullptr &&
                 pen != nullptr && finished != nullptr && hist != nullptr && hist_n2 != nullptr && winner != nullptr,
                 "contrastive_step: the hidden rows, the candidate arrays and the sentence state are required");
    const BeamArgs a = BEAM_COMMON_ARGS;
    const ContrastiveArgs ca{hidden, ld_h, d, alpha, min_len, max_c, cand_p, cand_score, ids, pen, len, hist, hist_n2, winner};
    return beam_dispatch("contrastive_step", k, [&](auto w) {
        hipLaunchKernelGGL(contrastive_step_kernel<decltype(w)::value>, dim3(n_sent), dim3(kBeamThreads), 0, stream, a, ca);
    });
}
