// Beam-search caption decoding (the reference's `--use_beam --beam_size B`, test.py:207-209 → translate.py:73-74 →
// Translator.translate_batch(use_beam=True), translator.py:194-203): one selection step over the B hypotheses of every sentence, and the
// final pick of the best hypothesis.  The decoder side (text embedding, layers, head, pointer-generator) is the greedy path's, run over the
// T·B hypothesis rows; the layers read each hypothesis's ancestry in the per-layer KV caches through the table written here
// (svpc_attn_q1_ln_idx_fwd), so the caches are never copied or reordered.
//
// Candidate order (a strict total order, restated by tests/beam_reference.py::select):
//   1. higher cum = cum_parent + step score,  2. higher raw value (p, or the logit in logits mode),  3. lower flat index parent·C + column.
// The step score is a monotone function of the raw value within a row (log p, or logit − log-sum-exp of the row), so a row's B best
// candidates by (raw, column) are its B best by the full order: one wave per row, every lane keeps a top-B of its columns by (raw, column)
// in registers, the 64 lanes merge by shuffle butterflies, and only the B·B survivors get a step score (computed in fp64 and
// rounded once, so the CPU reference reproduces it bit for bit).  UNK is not a candidate; a finished hypothesis (extended id EOS) offers
// exactly one: itself, token PAD, step score 0, raw value +inf.
#include "common.h"

#include <climits>

namespace {

constexpr int kBeamMax = 8;
constexpr int kBeamThreads = 256;

__device__ __forceinline__ bool raw_better(float v, int c, float w, int d) { return v > w || (v == w && c < d); }

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

__device__ __forceinline__ double wave_max_d(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

struct BeamArgs {
    const float* scores; int ld; const int* row_c; const int* row_x;
    int pos; int logits; int unk; int eos; int pad; int slot_rows;
    float* cum; int* finished;
    const int* text_in; const int* ext_in; const int* rows_in;
    int* text_out; int* ext_out; int* rows_out; int ld_tok;
    int* parent; int* next_ext; int* next_model;
};

template <int B>
__global__ __launch_bounds__(kBeamThreads) void beam_step_kernel(BeamArgs a) {
    constexpr int NC = B * B;                      // candidates that reach the final ranking (≤ 64: one lane each)
    __shared__ float c_cum[NC], c_raw[NC];
    __shared__ int c_flat[NC], c_par[NC], c_col[NC];
    __shared__ float p_cum[B];
    __shared__ int p_fin[B], n_cand;
    __shared__ int sel[B];
    const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r0 = t * B;
    if (tid < B) { p_cum[tid] = a.cum[r0 + tid]; p_fin[tid] = a.finished[r0 + tid]; }
    if (tid < NC) c_flat[tid] = INT_MAX;
    __syncthreads();
    // one wave per hypothesis row (B > 4: two rows per wave), the rows of a sentence side by side; no barrier inside a row
    for (int h = __builtin_amdgcn_readfirstlane(wave); h < B; h += kBeamThreads / 64) {
        const int r = r0 + h, C = a.row_c[r];
        if (p_fin[h]) {                           // (wave-uniform branch) a finished hypothesis carries itself forward
            if (lane == 0) {
                c_cum[h * B] = p_cum[h]; c_raw[h * B] = INFINITY; c_flat[h * B] = h * C + a.pad; c_par[h * B] = h; c_col[h * B] = a.pad;
            }
            continue;
        }
        const float* row = a.scores + (size_t)r * a.ld;
        double lse = 0.0;
        if (a.logits) {                           // log-sum-exp over the row's columns, UNK excluded (fp64)
            float m = -INFINITY;
            for (int c = lane; c < C; c += 64)
                if (c != a.unk) m = fmaxf(m, row[c]);
            const double md = wave_max_d((double)m);
            double sm = 0.0;
            for (int c = lane; c < C; c += 64)
                if (c != a.unk) sm += exp((double)row[c] - md);
            lse = md + log(wave_sum_d(sm));
        }
        float val[B]; int idx[B];
#pragma unroll
        for (int k = 0; k < B; ++k) { val[k] = -INFINITY; idx[k] = INT_MAX; }
        for (int c = lane; c < C; c += 64)
            if (c != a.unk) topb_insert<B>(val, idx, row[c], c);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {        // butterfly: lanes l and l^o hold disjoint sets, both end with their merged top-B
            float ov[B]; int oi[B];
#pragma unroll
            for (int k = 0; k < B; ++k) { ov[k] = __shfl_xor(val[k], o, 64); oi[k] = __shfl_xor(idx[k], o, 64); }
#pragma unroll
            for (int k = 0; k < B; ++k) topb_insert<B>(val, idx, ov[k], oi[k]);
        }
        if (lane < B) {                           // every lane holds the row's top-B: lane k keeps entry k
            float v = val[0]; int c = idx[0];
#pragma unroll
            for (int k = 1; k < B; ++k) if (lane == k) { v = val[k]; c = idx[k]; }
            if (c != INT_MAX) {
                float step;
                if (a.logits) step = (float)((double)v - lse);
                else step = v > 0.f ? (float)log((double)v) : -INFINITY;
                const int e = h * B + lane;
                c_cum[e] = p_cum[h] + step; c_raw[e] = v; c_flat[e] = h * C + c; c_par[e] = h; c_col[e] = c;
            }
        }
    }
    __syncthreads();
    if (tid < 64) {                               // rank every candidate against all others: the B best take slots 0 … B-1
        int rank = INT_MAX, n = 0;
        if (tid < NC && c_flat[tid] != INT_MAX) {
            const float cc = c_cum[tid], cr = c_raw[tid]; const int cf = c_flat[tid];
            rank = 0;
            for (int j = 0; j < NC; ++j) {
                if (c_flat[j] == INT_MAX) continue;
                const float oc = c_cum[j], orw = c_raw[j]; const int of = c_flat[j];
                rank += (oc > cc || (oc == cc && (orw > cr || (orw == cr && of < cf)))) ? 1 : 0;
            }
        }
        if (rank < B) sel[rank] = tid;
        n = __popcll(__ballot(tid < NC && c_flat[tid] != INT_MAX));
        if (tid == 0) n_cand = n;
    }
    __syncthreads();
    const int pl = a.pos + 1;                     // tokens of a child: its parent's positions 0 … pos, then its own pick at pos + 1
    if (tid < B) {
        const int r = r0 + tid;
        int h, col; float cu;
        if (tid < n_cand) { const int e = sel[tid]; h = c_par[e]; col = c_col[e]; cu = c_cum[e]; }
        else { h = tid; col = a.pad; cu = -INFINITY; }     // (fewer than B candidates: only when a row has < B columns besides UNK)
        const int C = a.row_c[r0 + h], X = a.row_x[r0 + h];
        const bool was_fin = p_fin[h] != 0 || tid >= n_cand;
        const int ext = was_fin ? a.pad : col;
        const int mod = was_fin ? a.pad : (col >= C - X ? a.unk : col);
        a.cum[r] = cu;
        a.finished[r] = (was_fin || ext == a.eos) ? 1 : 0;
        a.parent[r] = r0 + h;
        a.next_ext[r] = ext;
        a.next_model[r] = mod;
        a.text_out[(size_t)r * a.ld_tok + pl] = mod;
        a.ext_out[(size_t)r * a.ld_tok + pl] = ext;
        a.rows_out[(size_t)r * a.ld_tok + pl] = r * a.slot_rows + pl;
        sel[tid] = h;                             // (read below only after the barrier; every writer has read its entry)
    }
    __syncthreads();
    for (int e = tid; e < B * pl; e += kBeamThreads) {
        const int k = e / pl, j = e - k * pl;
        const size_t src = (size_t)(r0 + sel[k]) * a.ld_tok + j, dst = (size_t)(r0 + k) * a.ld_tok + j;
        a.text_out[dst] = a.text_in[src];
        a.ext_out[dst] = a.ext_in[src];
        a.rows_out[dst] = a.rows_in[src];
    }
}

__global__ __launch_bounds__(256) void beam_finalize_kernel(const float* __restrict__ cum, const int* __restrict__ ext, int ld_tok, int n_sent,
                                                            int B, int lt, int* __restrict__ best_ids, float* __restrict__ best_score) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_sent) return;
    int hb = 0; float cb = cum[(size_t)t * B];
    for (int h = 1; h < B; ++h) {
        const float c = cum[(size_t)t * B + h];
        if (c > cb) { cb = c; hb = h; }
    }
    best_score[t] = cb;
    const int* src = ext + (size_t)(t * B + hb) * ld_tok;
    for (int j = 0; j < lt; ++j) best_ids[(size_t)t * lt + j] = src[j];
}

}  // namespace

extern "C" {

int svpc_beam_step(const float* scores, int ld, const int* row_c, const int* row_x, int n_sent, int beam, int pos, int logits, int unk,
                   int eos, int pad, int slot_rows, float* cum, int* finished, const int* text_in, const int* ext_in, const int* rows_in,
                   int* text_out, int* ext_out, int* rows_out, int ld_tok, int* parent, int* next_ext, int* next_model,
                   hipStream_t stream) {
    if (n_sent == 0) return 0;
    SVPC_REQUIRE(beam >= 1 && beam <= kBeamMax, "beam_step: beam width must be 1..8");
    SVPC_REQUIRE(pos >= 0 && pos + 1 < ld_tok && pos + 1 < slot_rows, "beam_step: position pos + 1 must lie inside the token / ancestry rows");
    SVPC_REQUIRE(text_in != text_out && ext_in != ext_out && rows_in != rows_out, "beam_step: the token and ancestry tables are ping-pong pairs");
    BeamArgs a{scores, ld, row_c, row_x, pos, logits, unk, eos, pad, slot_rows, cum, finished, text_in, ext_in, rows_in,
               text_out, ext_out, rows_out, ld_tok, parent, next_ext, next_model};
    const dim3 grid(n_sent), block(kBeamThreads);
    switch (beam) {
        case 1: hipLaunchKernelGGL(beam_step_kernel<1>, grid, block, 0, stream, a); break;
        case 2: hipLaunchKernelGGL(beam_step_kernel<2>, grid, block, 0, stream, a); break;
        case 3: hipLaunchKernelGGL(beam_step_kernel<3>, grid, block, 0, stream, a); break;
        case 4: hipLaunchKernelGGL(beam_step_kernel<4>, grid, block, 0, stream, a); break;
        case 5: hipLaunchKernelGGL(beam_step_kernel<5>, grid, block, 0, stream, a); break;
        case 6: hipLaunchKernelGGL(beam_step_kernel<6>, grid, block, 0, stream, a); break;
        case 7: hipLaunchKernelGGL(beam_step_kernel<7>, grid, block, 0, stream, a); break;
        default: hipLaunchKernelGGL(beam_step_kernel<8>, grid, block, 0, stream, a); break;
    }
    return svpc_check_launch("beam_step");
}

int svpc_beam_finalize(const float* cum, const int* ext, int ld_tok, int n_sent, int beam, int lt, int* best_ids, float* best_score,
                       hipStream_t stream) {
    if (n_sent == 0) return 0;
    SVPC_REQUIRE(beam >= 1 && beam <= kBeamMax && lt >= 1 && lt <= ld_tok, "beam_finalize: beam width 1..8, 1 <= lt <= ld_tok");
    hipLaunchKernelGGL(beam_finalize_kernel, dim3((n_sent + 255) / 256), dim3(256), 0, stream, cum, ext, ld_tok, n_sent, beam, lt, best_ids,
                       best_score);
    return svpc_check_launch("beam_finalize");
}

}  // extern "C"
