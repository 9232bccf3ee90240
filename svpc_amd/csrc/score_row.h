// The row reduction behind a decoder step score, shared by beam.hip (svpc_beam_step) and force.hip (svpc_force_score) so that the step
// score of a column is the same number in both: the order of two candidates of one row, the fp64 log-sum-exp of a logits row without
// UNK (per lane the columns lane, lane + 64, … in that order, then a shuffle butterfly from offset 32 down), and the score itself,
// computed in fp64 and rounded once to fp32.
#pragma once
#include "common.h"

__device__ __forceinline__ bool raw_better(float v, int c, float w, int d) { return v > w || (v == w && c < d); }

__device__ __forceinline__ double wave_max_d(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// log-sum-exp of row[0 … C) without column unk, given this lane's maximum m of its columns (−inf: none); all 64 lanes call
__device__ __forceinline__ double row_lse_from_max(const float* row, int C, int unk, int lane, float m) {
    const double md = wave_max_d((double)m);
    double sm = 0.0;
    for (int c = lane; c < C; c += 64)
        if (c != unk) sm += exp((double)row[c] - md);
    return md + log(wave_sum_d(sm));
}

__device__ __forceinline__ double row_lse(const float* row, int C, int unk, int lane) {
    float m = -INFINITY;
    for (int c = lane; c < C; c += 64)
        if (c != unk) m = fmaxf(m, row[c]);
    return row_lse_from_max(row, C, unk, lane, m);
}

// step score of a column with raw value v: logit − lse (logits mode), else log p, −inf for p <= 0
__device__ __forceinline__ float step_score(float v, int logits, double lse) {
    if (logits) return (float)((double)v - lse);
    return v > 0.f ? (float)log((double)v) : -INFINITY;
}
