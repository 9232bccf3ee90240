// Diverse (group) beam search: the selection step (Vijayakumar et al. 2016, "Diverse Beam Search", arXiv 1610.02424; fairseq's
// --diverse-beam-groups / --diverse-beam-strength, Hamming diversity).  The W hypothesis rows of a sentence are G groups of Bg = W / G rows:
// row g·Bg + j is hypothesis j of group g.  The groups pick in order at every step, and a child (h, c) of group g pays pen[n] for the n rows
// of groups 0 … g − 1 whose live pick at this step is the word c (a live pick: a word chosen from an unfinished parent; the PAD a finished
// parent carries forward and a fill row do not count, EOS does).  Hypotheses never cross groups.  Restated by tests/diverse_beam_reference.py.
//
// Two scores per row: cum, the model's summed step scores (what svpc_beam_step_ctl keeps, what the decode returns), and aug, the selection
// score: cum minus every penalty paid on the way.  A child has cum' = fp32(cum_h + step), aug' = fp32(fp32(aug_h + step) − pen[n]) and
// ranks by key = (double)aug' / lp[p] (lp null: aug'); a finished parent offers itself, token PAD, cum / aug / len kept, key
// (double)aug / lp[len], raw value +inf, no penalty.  Group g's candidates — those of its Bg parents — rank by higher key, then higher raw
// value, then lower flat index h·C + c (h the parent's row in the sentence, 0 … W − 1); the Bg best become rows g·Bg … g·Bg + Bg − 1, and
// slots without a candidate are filled as in svpc_beam_step (parent the slot itself, PAD, cum = aug = −inf, finished, len p).  pen is a host
// table (pen[n] = fp32(fp32(λ)·n), n < W): the kernel never multiplies by λ, so no contraction into an fma can change a bit.
//
// Pruning: a penalised key is no longer monotone in the raw value within a row, but at most W − Bg distinct words carry a penalty, so a
// column outside its row's top-W by (raw, column) has at least W better columns of which at least Bg are unpenalised: every row's top-W by
// (raw, column) contains its top-Bg by penalised key, for every group.  So phase one is svpc_beam_step_ctl's with B = W — one wave per row,
// register top-W, shuffle butterflies, an fp64 step score rounded once for the ≤ W·W survivors, left in LDS.  Phase two is one wave: lane
// l holds candidate l of the current group (≤ Bg·W ≤ 64), counts its word among the picks of the earlier groups (lane i < W keeps the live
// pick of output row i in a register), ranks itself against the group's other candidates by shuffles, and the Bg winners move to the lanes
// of their output rows — no barrier between groups, no LDS or global traffic.  Phase three copies the parents' token and ancestry rows.
#include "beam_common.h"

namespace {

struct GroupArgs { int groups; const float* pen; float* aug; };

template <int W>
__global__ __launch_bounds__(kBeamThreads) void beam_step_groups_kernel(BeamArgs a, GroupArgs ga) {
    constexpr int NC = W * W;                      // survivors: the top-W columns of every row (≤ 64)
    __shared__ float c_step[NC], c_raw[NC];
    __shared__ int c_flat[NC], c_col[NC];
    __shared__ float p_cum[W], p_aug[W];
    __shared__ int p_fin[W], p_len[W];
    __shared__ int sel[W];
    __shared__ int ban[W][64], n_ban[W];           // n-gram blocking: the banned words of every live row
    const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r0 = t * W;
    const int pl = a.pos + 1;                      // position p of this step's pick
    if (tid < W) {
        p_cum[tid] = a.cum[r0 + tid]; p_aug[tid] = ga.aug[r0 + tid]; p_fin[tid] = a.finished[r0 + tid]; p_len[tid] = a.len[r0 + tid];
    }
    if (tid < NC) c_flat[tid] = INT_MAX;
    if (a.ngram == 0 || pl < a.ngram) {
        if (tid < W) n_ban[tid] = 0;
    } else {
        ngram_ban_rows<W>(a, r0, pl, lane, wave, ban, n_ban);
    }
    __syncthreads();
    const int skip_eos = pl <= a.min_len ? a.eos : a.unk;     // min length: EOS is skipped like UNK
    // phase one: one wave per hypothesis row, its top-W columns by (raw, column) and their step scores
    for (int h = __builtin_amdgcn_readfirstlane(wave); h < W; h += kBeamThreads / 64) {
        const int r = r0 + h, C = a.row_c[r];
        if (p_fin[h]) {                            // (wave-uniform branch) a finished hypothesis carries itself forward
            if (lane == 0) { c_step[h * W] = 0.f; c_raw[h * W] = INFINITY; c_flat[h * W] = h * C + a.pad; c_col[h * W] = a.pad; }
            continue;
        }
        const float* row = a.scores + (size_t)r * a.ld;
        const double lse = a.logits ? row_lse(row, C, a.unk, lane) : 0.0;
        float val[W]; int idx[W];
#pragma unroll
        for (int k = 0; k < W; ++k) { val[k] = -INFINITY; idx[k] = INT_MAX; }
        const int nb = n_ban[h];
        if (nb == 0) {
            for (int c = lane; c < C; c += 64)
                if (c != a.unk && c != skip_eos) topb_insert<W>(val, idx, row[c], c);
        } else {
            for (int c = lane; c < C; c += 64)
                if (c != a.unk && c != skip_eos) topb_insert_ban<W>(val, idx, row[c], c, ban[h], nb);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {         // butterfly: lanes l and l^o hold disjoint sets, both end with their merged top-W
            float ov[W]; int oi[W];
#pragma unroll
            for (int k = 0; k < W; ++k) { ov[k] = __shfl_xor(val[k], o, 64); oi[k] = __shfl_xor(idx[k], o, 64); }
#pragma unroll
            for (int k = 0; k < W; ++k) topb_insert<W>(val, idx, ov[k], oi[k]);
        }
        if (lane < W) {                            // every lane holds the row's top-W: lane k keeps entry k
            float v = val[0]; int c = idx[0];
#pragma unroll
            for (int k = 1; k < W; ++k) if (lane == k) { v = val[k]; c = idx[k]; }
            if (c != INT_MAX) {
                const int e = h * W + lane;
                c_step[e] = step_score(v, a.logits, lse); c_raw[e] = v; c_flat[e] = h * C + c; c_col[e] = c;
            }
        }
    }
    __syncthreads();
    // phase two: wave 0 walks the groups in order; everything between groups stays in its registers
    if (wave == 0) {
        const int G = ga.groups, Bg = W / G, ng = Bg * W;      // ng: the candidate entries of one group, one lane each
        int pick = -1;                             // lane i < W: the live pick of output row i at this step (−1: none, or not yet chosen)
        int o_par = lane < W ? lane : 0, o_col = a.pad, o_fin = 1, o_has = 0;
        float o_cum = -INFINITY, o_aug = -INFINITY;
        for (int g = 0; g < G; ++g) {
            const int e = g * ng + lane;
            const bool in = lane < ng;
            const int h = in ? e / W : 0;
            const int flat = in ? c_flat[e] : INT_MAX;
            const bool valid = flat != INT_MAX;
            const bool fin = valid && p_fin[h] != 0;
            const int col = valid ? c_col[e] : -2;
            int n = 0;                             // earlier groups' rows whose live pick is this word
            for (int i = 0; i < g * Bg; ++i) n += (__shfl(pick, i, 64) == col) ? 1 : 0;
            float cu = -INFINITY, au = -INFINITY, raw = -INFINITY;
            double key = -INFINITY;
            if (fin) {
                const int ln = min(max(p_len[h], 0), a.ld_tok - 1);
                cu = p_cum[h]; au = p_aug[h]; raw = INFINITY;
                key = a.lp ? (double)au / a.lp[ln] : (double)au;
            } else if (valid) {
                const float st = c_step[e];
                const float s = p_aug[h] + st;
                cu = p_cum[h] + st; au = s - ga.pen[n]; raw = c_raw[e];
                key = a.lp ? (double)au / a.lp[pl] : (double)au;
            }
            int rank = 0;                          // the group's candidates ahead of this one (a strict total order)
            for (int j = 0; j < ng; ++j) {
                const double ok = __shfl(key, j, 64); const float orw = __shfl(raw, j, 64); const int of = __shfl(flat, j, 64);
                rank += (of != INT_MAX && (ok > key || (ok == key && (orw > raw || (orw == raw && of < flat))))) ? 1 : 0;
            }
            if (!valid) rank = INT_MAX;
            for (int k = 0; k < Bg; ++k) {         // the winner of rank k moves to the lane of output row g·Bg + k
                const unsigned long long m = __ballot(rank == k);
                const int src = m ? __ffsll((long long)m) - 1 : 0;
                const int s_h = __shfl(h, src, 64), s_col = __shfl(col, src, 64), s_fin = __shfl((int)fin, src, 64);
                const float s_cu = __shfl(cu, src, 64), s_au = __shfl(au, src, 64);
                if (m && lane == g * Bg + k) {     // (no candidate of that rank: the slot keeps its fill values)
                    o_par = s_h; o_col = s_col; o_fin = s_fin; o_has = 1; o_cum = s_cu; o_aug = s_au;
                    pick = s_fin ? -1 : s_col;
                }
            }
        }
        // tokens of a child: its parent's positions 0 … pos, then its own pick at pos + 1
        if (lane < W) {
            const int r = r0 + lane, h = o_par;
            const int C = a.row_c[r0 + h], X = a.row_x[r0 + h];
            const bool was_fin = o_fin != 0;       // a finished parent, or a fill row
            const int ext = was_fin ? a.pad : o_col;
            const int mod = was_fin ? a.pad : (o_col >= C - X ? a.unk : o_col);
            a.cum[r] = o_cum;
            ga.aug[r] = o_aug;
            a.finished[r] = (was_fin || ext == a.eos) ? 1 : 0;
            a.len[r] = (o_has && p_fin[h]) ? p_len[h] : pl;     // a finished parent keeps its length
            a.parent[r] = r0 + h;
            a.next_ext[r] = ext;
            a.next_model[r] = mod;
            a.text_out[(size_t)r * a.ld_tok + pl] = mod;
            a.ext_out[(size_t)r * a.ld_tok + pl] = ext;
            a.rows_out[(size_t)r * a.ld_tok + pl] = r * a.slot_rows + pl;
            sel[lane] = h;
        }
    }
    __syncthreads();
    for (int e = tid; e < W * pl; e += kBeamThreads) {
        const int k = e / pl, j = e - k * pl;
        const size_t src = (size_t)(r0 + sel[k]) * a.ld_tok + j, dst = (size_t)(r0 + k) * a.ld_tok + j;
        a.text_out[dst] = a.text_in[src];
        a.ext_out[dst] = a.ext_in[src];
        a.rows_out[dst] = a.rows_in[src];
    }
}

}  // namespace

extern "C" int svpc_beam_step_groups(const float* scores, int ld, const int* row_c, const int* row_x, int n_sent, int beam, int pos, int logits,
                                     int unk, int eos, int pad, int slot_rows, float* cum, int* finished, const int* text_in,
                                     const int* ext_in, const int* rows_in, int* text_out, int* ext_out, int* rows_out, int ld_tok,
                                     int* parent, int* next_ext, int* next_model, int min_len, int ngram, const unsigned* excl, int excl_v,
                                     const double* lp, int* len, int groups, const float* pen, float* aug, hipStream_t stream) {
    if (n_sent == 0) return 0;
    SVPC_REQUIRE(beam >= 1 && beam <= kBeamMax, "beam_step_groups: beam width must be 1..8");
    SVPC_REQUIRE(groups >= 1 && beam % groups == 0, "beam_step_groups: the number of groups must divide the beam width");
    SVPC_REQUIRE(pos >= 0 && pos + 1 < ld_tok && pos + 1 < slot_rows, "beam_step_groups: position pos + 1 must lie inside the token / ancestry rows");
    SVPC_REQUIRE(text_in != text_out && ext_in != ext_out && rows_in != rows_out, "beam_step_groups: the token and ancestry tables are ping-pong pairs");
    SVPC_REQUIRE(min_len >= 0 && min_len < ld_tok && ngram >= 0 && ngram < ld_tok, "beam_step_groups: min length and n-gram size must be 0..ld_tok-1");
    SVPC_REQUIRE(ngram == 0 || ld_tok <= 64, "beam_step_groups: n-gram blocking holds a hypothesis's ids in one wave (ld_tok <= 64)");
    SVPC_REQUIRE(len != nullptr && pen != nullptr && aug != nullptr, "beam_step_groups: the length array, the penalty table and aug are required");
    SVPC_REQUIRE(excl == nullptr || excl_v > 0, "beam_step_groups: the exclusion bitmap needs its id count");
    BeamArgs a{scores, ld, row_c, row_x, pos, logits, unk, eos, pad, slot_rows, cum, finished, text_in, ext_in, rows_in,
               text_out, ext_out, rows_out, ld_tok, parent, next_ext, next_model, min_len, ngram, excl, excl_v, lp, len, nullptr, nullptr, 0};
    GroupArgs ga{groups, pen, aug};
    const dim3 grid(n_sent), block(kBeamThreads);
    switch (beam) {
        case 1: hipLaunchKernelGGL((beam_step_groups_kernel<1>), grid, block, 0, stream, a, ga); break;
        case 2: hipLaunchKernelGGL((beam_step_groups_kernel<2>), grid, block, 0, stream, a, ga); break;
        case 3: hipLaunchKernelGGL((beam_step_groups_kernel<3>), grid, block, 0, stream, a, ga); break;
        case 4: hipLaunchKernelGGL((beam_step_groups_kernel<4>), grid, block, 0, stream, a, ga); break;
        case 5: hipLaunchKernelGGL((beam_step_groups_kernel<5>), grid, block, 0, stream, a, ga); break;
        case 6: hipLaunchKernelGGL((beam_step_groups_kernel<6>), grid, block, 0, stream, a, ga); break;
        case 7: hipLaunchKernelGGL((beam_step_groups_kernel<7>), grid, block, 0, stream, a, ga); break;
        default: hipLaunchKernelGGL((beam_step_groups_kernel<8>), grid, block, 0, stream, a, ga); break;
    }
    return svpc_check_launch("beam_step_groups");
}
