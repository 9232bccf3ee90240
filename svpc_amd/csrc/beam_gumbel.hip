// Stochastic beam search (Kool, van Hoof and Welling 2019, "Stochastic Beams and Where to Find Them", arXiv 1903.06059): one selection step
// over the W rows of every sentence — a beam search over Gumbel-perturbed log-probabilities whose W rows are an exact sample WITHOUT
// replacement from the model's sequence distribution, in the order in which they were drawn.  The decoder side, the ping-pong id and
// ancestry tables and the launch shape are the beam decode's (beam.hip); the draw is sampling's counter-based one (sample.hip).
//
// Every row carries cum (fp32, the model's summed step score, as beam's), phi (fp64, the log-probability of its sequence under the tempered,
// renormalised model), G (fp64, the perturbed log-probability), finished and len.  A dead row is finished with G = −inf.  One step at
// position p = pos + 1 (restated by tests/stochastic_beam_reference.py::stochastic_beam_select):
//   K0    of a live row h (global row r = t·W + h): columns c < C_r, c ≠ UNK, step score s_c > −inf, not EOS while p ≤ min_len;
//   z_c   = (double)s_c / τ, s_c beam's step score (fp64, rounded once to fp32);  L = m + log Σ_K0 exp(z_c − m), m = max z;
//   φ_c   = phi_h + (z_c − L);  g_c = φ_c − log(−log u_c), u_c = (svpc_hash32(seed, pos, r·4096 + c) + 0.5)·2⁻³²;
//   short list: the row's first W candidates by higher g, then lower c; Z_h the first one's g;
//   G̃_c   = G_h − max(v, 0) − log1p(exp(−|v|)), v = G_h − g_c + log1p(−exp(g_c − Z_h)) (the truncated-Gumbel transform, appendix B.3);
//   a finished row with finite G offers itself: PAD, step score 0, G̃ = g = G_h, flat index h·4096 + PAD; a dead row offers nothing;
//   the sentence's new rows 0 … W − 1 are its first W candidates by higher G̃, then higher g, then lower flat index h·4096 + c;
//   child: cum = fp32(cum_h + s_c), phi = φ_c, G = G̃_c, len = p, finished on EOS; leftover slots are dead rows (PAD, −inf, len p).
// G̃ is non-decreasing in g within a row, so the W·W short-listed candidates hold the sentence's W best.
//
// One 256-thread workgroup per sentence, one wave per parent row (W > 4: two rows per wave).  The row is read three times (it stays in
// the cache): the largest raw value among K0 (z is monotone in it, so m is its z), Σ exp(z − m), then every lane forms g for its columns
// and keeps a register top-W by (g, column); the 64 lanes merge by a shuffle butterfly; the ≤ W·W survivors get the transform and are
// ranked from LDS as beam_step_kernel ranks its B·B survivors.
#include "beam_common.h"

namespace {

constexpr int kGumbelCols = 4096;                  // the column stride of the draw index r·4096 + c and of the flat index h·4096 + c

struct GumbelArgs {
    const float* scores; int ld; const int* row_c; const int* row_x;
    int pos; int logits; int unk; int eos; int pad; int slot_rows;
    float* cum; int* finished;
    const int* text_in; const int* ext_in; const int* rows_in;
    int* text_out; int* ext_out; int* rows_out; int ld_tok;
    int* parent; int* next_ext; int* next_model;
    double temp; int min_len; const long long* seed; double* phi; double* gkey; int* len; int max_c;
};

template <int B>
__global__ __launch_bounds__(kBeamThreads) void beam_step_gumbel_kernel(GumbelArgs a) {
    constexpr int NC = B * B;                      // candidates that reach the final ranking (≤ 64: one lane each)
    __shared__ double c_gt[NC], c_g[NC], c_phi[NC];
    __shared__ float c_cum[NC];
    __shared__ int c_flat[NC], c_par[NC], c_col[NC];
    __shared__ double p_phi[B], p_g[B];
    __shared__ float p_cum[B];
    __shared__ int p_fin[B], p_len[B], n_cand;
    __shared__ int sel[B];
    const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r0 = t * B;
    const int pl = a.pos + 1;                     // position p of this step's pick
    if (tid < B) {
        p_cum[tid] = a.cum[r0 + tid]; p_fin[tid] = a.finished[r0 + tid]; p_len[tid] = a.len[r0 + tid];
        p_phi[tid] = a.phi[r0 + tid]; p_g[tid] = a.gkey[r0 + tid];
    }
    if (tid < NC) c_flat[tid] = INT_MAX;
    __syncthreads();
    const int skip_eos = pl <= a.min_len ? a.eos : a.unk;     // min length: EOS is skipped like UNK
    const u64 seed = (u64)a.seed[0];
    for (int h = __builtin_amdgcn_readfirstlane(wave); h < B; h += kBeamThreads / 64) {
        const int r = r0 + h;
        if (p_fin[h]) {                           // (wave-uniform branch) a finished row carries itself forward; a dead one offers nothing
            if (lane == 0 && p_g[h] > -INFINITY) {
                c_gt[h * B] = p_g[h]; c_g[h * B] = p_g[h]; c_phi[h * B] = p_phi[h]; c_cum[h * B] = p_cum[h];
                c_flat[h * B] = h * kGumbelCols + a.pad; c_par[h * B] = h; c_col[h * B] = a.pad;
            }
            continue;
        }
        const int C = min(a.row_c[r], a.max_c);
        const float* row = a.scores + (size_t)r * a.ld;
        const double lse = a.logits ? row_lse(row, C, a.unk, lane) : 0.0;     // beam's log-sum-exp: the step score has beam.hip's bits
        float mr = -INFINITY;                     // the largest raw value among the allowed columns: its z is m
        for (int c = lane; c < C; c += 64)
            if (c != a.unk && c != skip_eos) mr = fmaxf(mr, row[c]);
        mr = wave_max(mr);
        const float sm = step_score(mr, a.logits, lse);
        if (!(sm > -INFINITY)) continue;          // (wave-uniform) an empty K0: the row offers nothing
        const double m = (double)sm / a.temp;
        double sum = 0.0;
        for (int c = lane; c < C; c += 64) {
            if (c == a.unk || c == skip_eos) continue;
            const float s = step_score(row[c], a.logits, lse);
            if (s > -INFINITY) sum += exp((double)s / a.temp - m);
        }
        const double L = m + log(wave_sum_d(sum));
        const double ph = p_phi[h];
        double val[B]; int idx[B];
#pragma unroll
        for (int k = 0; k < B; ++k) { val[k] = -INFINITY; idx[k] = INT_MAX; }
        for (int c = lane; c < C; c += 64) {
            if (c == a.unk || c == skip_eos) continue;
            const float s = step_score(row[c], a.logits, lse);
            if (!(s > -INFINITY)) continue;
            const uint32_t hs = svpc_hash32(seed, (uint32_t)a.pos, (u64)r * kGumbelCols + (u64)c);
            const double u = ((double)hs + 0.5) * (1.0 / 4294967296.0);
            const double g = (ph + ((double)s / a.temp - L)) - log(-log(u));
            topb_insert_key<B>(val, idx, g, c);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {        // butterfly: lanes l and l^o hold disjoint sets, both end with their merged top-B
            double ov[B]; int oi[B];
#pragma unroll
            for (int k = 0; k < B; ++k) { ov[k] = __shfl_xor(val[k], o, 64); oi[k] = __shfl_xor(idx[k], o, 64); }
#pragma unroll
            for (int k = 0; k < B; ++k) topb_insert_key<B>(val, idx, ov[k], oi[k]);
        }
        if (lane < B) {                           // every lane holds the row's short list: lane k keeps entry k
            double g = val[0]; int c = idx[0];
#pragma unroll
            for (int k = 1; k < B; ++k) if (lane == k) { g = val[k]; c = idx[k]; }
            if (c != INT_MAX) {
                const float s = step_score(row[c], a.logits, lse);
                const double G = p_g[h];
                const double v = G - g + log1p(-exp(g - val[0]));
                const int e = h * B + lane;
                c_gt[e] = G - fmax(v, 0.0) - log1p(exp(-fabs(v)));
                c_g[e] = g; c_phi[e] = ph + ((double)s / a.temp - L); c_cum[e] = p_cum[h] + s;
                c_flat[e] = h * kGumbelCols + c; c_par[e] = h; c_col[e] = c;
            }
        }
    }
    __syncthreads();
    if (tid < 64) {                               // rank every candidate against all others: the B best take slots 0 … B-1
        int rank = INT_MAX;
        const bool live = tid < NC && c_flat[tid] != INT_MAX;
        if (live) {
            const double ck = c_gt[tid], cg = c_g[tid]; const int cf = c_flat[tid];
            rank = 0;
            for (int j = 0; j < NC; ++j) {
                if (c_flat[j] == INT_MAX) continue;
                const double ok = c_gt[j], og = c_g[j]; const int of = c_flat[j];
                rank += (ok > ck || (ok == ck && (og > cg || (og == cg && of < cf)))) ? 1 : 0;
            }
        }
        if (rank < B) sel[rank] = tid;
        const int n = __popcll(__ballot(live));
        if (tid == 0) n_cand = n;
    }
    __syncthreads();
    // tokens of a child: its parent's positions 0 … pos, then its own pick at pos + 1
    if (tid < B) {
        const int r = r0 + tid;
        int h, col; float cu; double ph, gt;
        if (tid < n_cand) { const int e = sel[tid]; h = c_par[e]; col = c_col[e]; cu = c_cum[e]; ph = c_phi[e]; gt = c_gt[e]; }
        else { h = tid; col = a.pad; cu = -INFINITY; ph = -INFINITY; gt = -INFINITY; }     // (fewer than B candidates: a dead row)
        const int C = min(a.row_c[r0 + h], a.max_c), X = a.row_x[r0 + h];
        const bool was_fin = p_fin[h] != 0 || tid >= n_cand;
        const int ext = was_fin ? a.pad : col;
        const int mod = was_fin ? a.pad : (col >= C - X ? a.unk : col);
        a.cum[r] = cu; a.phi[r] = ph; a.gkey[r] = gt;
        a.finished[r] = (was_fin || ext == a.eos) ? 1 : 0;
        a.len[r] = (tid < n_cand && p_fin[h]) ? p_len[h] : pl;    // a finished parent keeps its length
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

}  // namespace

extern "C" int svpc_beam_step_gumbel(const float* scores, int ld, const int* row_c, const int* row_x, int n_sent, int beam, int pos,
                                     int logits, int unk, int eos, int pad, int slot_rows, float* cum, int* finished, const int* text_in,
                                     const int* ext_in, const int* rows_in, int* text_out, int* ext_out, int* rows_out, int ld_tok,
                                     int* parent, int* next_ext, int* next_model, double temp, int min_len, const long long* seed,
                                     double* phi, double* gkey, int* len, int max_c, hipStream_t stream) {
    if (n_sent == 0) return 0;
    SVPC_REQUIRE(beam >= 1 && beam <= kBeamMax, "beam_step_gumbel: beam width must be 1..8");
    SVPC_REQUIRE(pos >= 0 && pos + 1 < ld_tok && pos + 1 < slot_rows, "beam_step_gumbel: position pos + 1 must lie inside the token / ancestry rows");
    SVPC_REQUIRE(text_in != text_out && ext_in != ext_out && rows_in != rows_out, "beam_step_gumbel: the token and ancestry tables are ping-pong pairs");
    SVPC_REQUIRE(max_c >= 1 && max_c <= kGumbelCols && max_c <= ld, "beam_step_gumbel: row columns must be 1..4096 and within ld");
    SVPC_REQUIRE(temp > 0.0 && temp <= 1.7976931348623157e308, "beam_step_gumbel: temperature must be finite and > 0");
    SVPC_REQUIRE(min_len >= 0 && min_len < ld_tok, "beam_step_gumbel: min length must be 0..ld_tok-1");
    SVPC_REQUIRE(seed != nullptr && phi != nullptr && gkey != nullptr && len != nullptr,
                 "beam_step_gumbel: the seed word and the phi, G and length arrays are required");
    GumbelArgs a{scores, ld, row_c, row_x, pos, logits, unk, eos, pad, slot_rows, cum, finished, text_in, ext_in, rows_in,
                 text_out, ext_out, rows_out, ld_tok, parent, next_ext, next_model, temp, min_len, seed, phi, gkey, len, max_c};
    const dim3 grid(n_sent), block(kBeamThreads);
    switch (beam) {
        case 1: hipLaunchKernelGGL(beam_step_gumbel_kernel<1>, grid, block, 0, stream, a); break;
        case 2: hipLaunchKernelGGL(beam_step_gumbel_kernel<2>, grid, block, 0, stream, a); break;
        case 3: hipLaunchKernelGGL(beam_step_gumbel_kernel<3>, grid, block, 0, stream, a); break;
        case 4: hipLaunchKernelGGL(beam_step_gumbel_kernel<4>, grid, block, 0, stream, a); break;
        case 5: hipLaunchKernelGGL(beam_step_gumbel_kernel<5>, grid, block, 0, stream, a); break;
        case 6: hipLaunchKernelGGL(beam_step_gumbel_kernel<6>, grid, block, 0, stream, a); break;
        case 7: hipLaunchKernelGGL(beam_step_gumbel_kernel<7>, grid, block, 0, stream, a); break;
        default: hipLaunchKernelGGL(beam_step_gumbel_kernel<8>, grid, block, 0, stream, a); break;
    }
    return svpc_check_launch("beam_step_gumbel");
}
