// What the beam-search selection kernels share (beam.hip: svpc_beam_step / _ctl / _para; beam_groups.hip: svpc_beam_step_groups): the
// launch shape, the kernel arguments, the register top-B insertion of a lane's columns, and the sentence-scope n-gram ban pass — so that a
// row's survivors and its banned words are the same in both.
#pragma once
#include "common.h"
#include "score_row.h"

#include <climits>

constexpr int kBeamMax = 8;
constexpr int kBeamThreads = 256;

// insert (v, c) into the sorted top-B list (val, idx); entries past the last real one hold (-inf, INT_MAX)
template <int B>
__device__ __forceinline__ void topb_insert(float (&val)[B], int (&idx)[B], float v, int c) {
    if (!raw_better(v, c, val[B - 1], idx[B - 1])) return;
#pragma unroll
    for (int k = 0; k < B; ++k) {
        if (raw_better(v, c, val[k], idx[k])) {
            const float tv = val[k]; const int ti = idx[k];
            val[k] = v; idx[k] = c; v = tv; c = ti;
        }
    }
}

// the same list with an fp64 key (beam_gumbel.hip: the perturbed log-probability g of a column): higher key, then lower column
__device__ __forceinline__ bool key_better(double v, int c, double w, int d) { return v > w || (v == w && c < d); }

template <int B>
__device__ __forceinline__ void topb_insert_key(double (&val)[B], int (&idx)[B], double v, int c) {
    if (!key_better(v, c, val[B - 1], idx[B - 1])) return;
#pragma unroll
    for (int k = 0; k < B; ++k) {
        if (key_better(v, c, val[k], idx[k])) {
            const double tv = val[k]; const int ti = idx[k];
            val[k] = v; idx[k] = c; v = tv; c = ti;
        }
    }
}

struct BeamArgs {
    const float* scores; int ld; const int* row_c; const int* row_x;
    int pos; int logits; int unk; int eos; int pad; int slot_rows;
    float* cum; int* finished;
    const int* text_in; const int* ext_in; const int* rows_in;
    int* text_out; int* ext_out; int* rows_out; int ld_tok;
    int* parent; int* next_ext; int* next_model;
    int min_len; int ngram; const unsigned* excl; int excl_v; const double* lp; int* len;    // controls (0 / null: off)
    const int* hist; const int* hdesc; int bos;                                            // paragraph scope (PARA only)
};

// the top-B insertion of a row with banned words (ban[0 … nb), a short LDS list): the list is read only by a column that would enter
template <int B>
__device__ __forceinline__ void topb_insert_ban(float (&val)[B], int (&idx)[B], float v, int c, const int* ban, int nb) {
    if (!raw_better(v, c, val[B - 1], idx[B - 1])) return;
    for (int k = 0; k < nb; ++k)
        if (ban[k] == c) return;
    topb_insert<B>(val, idx, v, c);
}

__device__ __forceinline__ bool excluded(const BeamArgs& a, int y) {
    return a.excl != nullptr && y >= 0 && y < a.excl_v && ((a.excl[y >> 5] >> (y & 31)) & 1u);
}

// n-gram blocking, sentence scope: the banned words of every live row h of the sentence whose rows start at r0, into ban[h][0 … n_ban[h]).
// Called by the whole workgroup when the step blocks (a.ngram > 0, pl >= a.ngram); one wave per row, lane l holds y_l, one lane per start
// j = 1 … p − n of an earlier gram.  The caller's barrier publishes the lists.
template <int B>
__device__ __forceinline__ void ngram_ban_rows(const BeamArgs& a, int r0, int pl, int lane, int wave, int (*ban)[64], int* n_ban) {
    const int n = a.ngram, s0 = pl - n + 1;   // the (n − 1)-suffix y_{s0} … y_pos of the new gram
    for (int h = __builtin_amdgcn_readfirstlane(wave); h < B; h += kBeamThreads / 64) {
        if (a.finished[r0 + h]) {             // (wave-uniform; the row's wave is the only writer of n_ban[h] before the barrier)
            if (lane == 0) n_ban[h] = 0;
            continue;
        }
        const int y = lane <= a.pos ? a.ext_in[(size_t)(r0 + h) * a.ld_tok + lane] : -1;
        const bool ex = excluded(a, y);
        const bool suffix_ex = __ballot(ex && lane >= s0 && lane <= a.pos) != 0ull;
        bool match = lane >= 1 && lane <= pl - n;
        for (int k = 0; k < n - 1; ++k) match &= __shfl(y, lane + k, 64) == __shfl(y, s0 + k, 64);
        const int w = __shfl(y, lane + n - 1, 64);
        const bool w_ex = __shfl((int)ex, lane + n - 1, 64) != 0;
        const bool banned = match && !suffix_ex && !w_ex;
        const unsigned long long m = __ballot(banned);
        if (banned) ban[h][__popcll(m & ((1ull << lane) - 1ull))] = w;
        if (lane == 0) n_ban[h] = __popcll(m);
    }
}
