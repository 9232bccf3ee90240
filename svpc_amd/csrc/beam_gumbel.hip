// Stochastic beam search (Kool, van Hoof and Welling 2019, "Stochastic Beams and Where to Find Them", arXiv 1903.06059): one selection step
// over the W rows of every sentence — a beam search over Gumbel-perturbed log-probabilities whose W rows are an exact sample WITHOUT
// replacement from the model's sequence distribution, in the order in which they were drawn.  The decoder side, the ping-pong id and ancestry
// tables, the launch shape and the kernel's skeleton are the beam decode's (beam_common.h); the draw is sampling's counter-based one
// (sample.hip).
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

struct GumbelArgs { double temp; int min_len; const long long* seed; double* phi; double* gkey; int* len; int max_c; };

template <int B>
__global__ __launch_bounds__(kBeamThreads) void beam_step_gumbel_kernel(BeamArgs a, GumbelArgs ga) {
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
    load_parents<B>(a, ga.len, r0, tid, p_cum, p_fin, p_len);
    if (tid < B) { p_phi[tid] = ga.phi[r0 + tid]; p_g[tid] = ga.gkey[r0 + tid]; }
    if (tid < NC) c_flat[tid] = INT_MAX;
    __syncthreads();
    const int skip_eos = pl <= ga.min_len ? a.eos : a.unk;     // min length: EOS is skipped like UNK
    const u64 seed = (u64)ga.seed[0];
    for (int h = __builtin_amdgcn_readfirstlane(wave); h < B; h += kBeamThreads / 64) {
        const int r = r0 + h;
        if (p_fin[h]) {                           // (wave-uniform branch) a finished row carries itself forward; a dead one offers nothing
            if (lane == 0 && p_g[h] > -INFINITY) {
                c_gt[h * B] = p_g[h]; c_g[h * B] = p_g[h]; c_phi[h * B] = p_phi[h]; c_cum[h * B] = p_cum[h];
                c_flat[h * B] = h * kGumbelCols + a.pad; c_par[h * B] = h; c_col[h * B] = a.pad;
            }
            continue;
        }
        const int C = min(a.row_c[r], ga.max_c);
        const float* row = a.scores + (size_t)r * a.ld;
        const double lse = a.logits ? row_lse(row, C, a.unk, lane) : 0.0;     // beam's log-sum-exp: the step score has beam.hip's bits
        float mr = -INFINITY;                     // the largest raw value among the allowed columns: its z is m
        for (int c = lane; c < C; c += 64)
            if (c != a.unk && c != skip_eos) mr = fmaxf(mr, row[c]);
        mr = wave_max(mr);
        const float sm = step_score(mr, a.logits, lse);
        if (!(sm > -INFINITY)) continue;          // (wave-uniform) an empty K0: the row offers nothing
        const double m = (double)sm / ga.temp;
        double sum = 0.0;
        for (int c = lane; c < C; c += 64) {
            if (c == a.unk || c == skip_eos) continue;
            const float s = step_score(row[c], a.logits, lse);
            if (s > -INFINITY) sum += exp((double)s / ga.temp - m);
        }
        const double L = m + log(wave_sum_d(sum));
        const double ph = p_phi[h];
        double val[B]; int idx[B];
        topb_row<B>(val, idx, C, lane, a.unk, skip_eos, [&](int c, double& g) {
            const float s = step_score(row[c], a.logits, lse);
            if (!(s > -INFINITY)) return false;
            const uint32_t hs = svpc_hash32(seed, (uint32_t)a.pos, (u64)r * kGumbelCols + (u64)c);
            const double u = ((double)hs + 0.5) * (1.0 / 4294967296.0);
            g = (ph + ((double)s / ga.temp - L)) - log(-log(u));
            return true;
        }, NoBan{});
        if (lane < B) {                           // the row's short list: val[0] is Z_h
            double g; int c;
            topb_entry<B>(val, idx, lane, g, c);
            if (c != INT_MAX) {
                const float s = step_score(row[c], a.logits, lse);
                const double G = p_g[h];
                const double v = G - g + log1p(-exp(g - val[0]));
                const int e = h * B + lane;
                c_gt[e] = G - fmax(v, 0.0) - log1p(exp(-fabs(v)));
                c_g[e] = g; c_phi[e] = ph + ((double)s / ga.temp - L); c_cum[e] = p_cum[h] + s;
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
    if (tid < B) {
        const int r = r0 + tid;
        int h, col; float cu; double ph, gt;
        if (tid < n_cand) { const int e = sel[tid]; h = c_par[e]; col = c_col[e]; cu = c_cum[e]; ph = c_phi[e]; gt = c_gt[e]; }
        else { h = tid; col = a.pad; cu = -INFINITY; ph = -INFINITY; gt = -INFINITY; }     // (fewer than B candidates: a dead row)
        const bool kept = tid < n_cand && p_fin[h];       // a finished parent keeps its length
        write_child(a, ga.len, pl, r, r0 + h, col, p_fin[h] != 0 || tid >= n_cand, cu, kept ? p_len[h] : pl, ga.max_c);
        ga.phi[r] = ph; ga.gkey[r] = gt;
        sel[tid] = h;                             // (read below only after the barrier; every writer has read its entry)
    }
    __syncthreads();
    copy_parent_rows<B>(a, r0, pl, tid, sel);
}

}  // namespace

extern "C" int svpc_beam_step_gumbel(const float* scores, int ld, const int* row_c, const int* row_x, int n_sent, int beam, int pos,
                                     int logits, int unk, int eos, int pad, int slot_rows, float* cum, int* finished, const int* text_in,
                                     const int* ext_in, const int* rows_in, int* text_out, int* ext_out, int* rows_out, int ld_tok,
                                     int* parent, int* next_ext, int* next_model, double temp, int min_len, const long long* seed,
                                     double* phi, double* gkey, int* len, int max_c, hipStream_t stream) {
    if (n_sent == 0) return 0;
    BEAM_REQUIRE_COMMON("beam_step_gumbel");
    SVPC_REQUIRE(max_c >= 1 && max_c <= kGumbelCols && max_c <= ld, "beam_step_gumbel: row columns must be 1..4096 and within ld");
    SVPC_REQUIRE(temp > 0.0 && temp <= 1.7976931348623157e308, "beam_step_gumbel: temperature must be finite and > 0");
    SVPC_REQUIRE(min_len >= 0 && min_len < ld_tok, "beam_step_gumbel: min length must be 0..ld_tok-1");
    SVPC_REQUIRE(seed != nullptr && phi != nullptr && gkey != nullptr && len != nullptr,
                 "beam_step_gumbel: the seed word and the phi, G and length arrays are required");
    const BeamArgs a = BEAM_COMMON_ARGS;
    const GumbelArgs ga{temp, min_len, seed, phi, gkey, len, max_c};
    return beam_dispatch("beam_step_gumbel", beam, [&](auto w) {
        hipLaunchKernelGGL(beam_step_gumbel_kernel<decltype(w)::value>, dim3(n_sent), dim3(kBeamThreads), 0, stream, a, ga);
    });
}
