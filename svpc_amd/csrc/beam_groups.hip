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
// slots without a candidate are fill rows (beam_common.h: write_child; parent the slot itself, PAD, cum = aug = −inf, finished, len p).
// pen is a host table (pen[n] = fp32(fp32(λ)·n), n < W): the kernel never multiplies by λ, so no contraction into an fma can change a bit.
//
// Pruning: a penalised key is no longer monotone in the raw value within a row, but at most W − Bg distinct words carry a penalty, so a
// column outside its row's top-W by (raw, column) has at least W better columns of which at least Bg are unpenalised: every row's top-W by
// (raw, column) contains its top-Bg by penalised key, for every group.  So phase one is beam_common.h's topb_row with B = W — one wave per
// row, register top-W, shuffle butterflies — and an fp64 step score rounded once for the ≤ W·W survivors, left in LDS.  Phase two is one
// wave: lane
// l holds candidate l of the current group (≤ Bg·W ≤ 64), counts its word among the picks of the earlier groups (lane i < W keeps the live
// pick of output row i in a register), ranks itself against the group's other candidates by shuffles, and the Bg winners move to the lanes
// of their output rows — no barrier between groups, no LDS or global traffic.  Phase three copies the parents' token and ancestry rows.
#include "beam_common.h"

namespace {

struct GroupArgs { int groups; const float* pen; float* aug; };

template <int W>
__global__ __launch_bounds__(kBeamThreads) void beam_step_groups_kernel(BeamArgs a, BeamCtl ctl, GroupArgs ga) {
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
    load_parents<W>(a, ctl.len, r0, tid, p_cum, p_fin, p_len);
    if (tid < W) p_aug[tid] = ga.aug[r0 + tid];
    if (tid < NC) c_flat[tid] = INT_MAX;
    ngram_bans<W>(a, ctl, r0, pl, tid, ban, n_ban);
    __syncthreads();
    const int skip_eos = pl <= ctl.min_len ? a.eos : a.unk;     // min length: EOS is skipped like UNK
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
        topb_row<W>(val, idx, C, lane, a.unk, skip_eos, RawKey{row}, BanList{ban[h], n_ban[h]});
        if (lane < W) {
            float v; int c;
            topb_entry<W>(val, idx, lane, v, c);
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
                key = ctl.lp ? (double)au / ctl.lp[ln] : (double)au;
            } else if (valid) {
                const float st = c_step[e];
                const float s = p_aug[h] + st;
                cu = p_cum[h] + st; au = s - ga.pen[n]; raw = c_raw[e];
                key = ctl.lp ? (double)au / ctl.lp[pl] : (double)au;
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
        if (lane < W) {
            const int r = r0 + lane, h = o_par;
            const bool kept = o_has && p_fin[h];  // a finished parent keeps its length
            write_child(a, ctl.len, pl, r, r0 + h, o_col, o_fin != 0, o_cum, kept ? p_len[h] : pl);     // (o_fin: a finished parent, or a fill row)
            ga.aug[r] = o_aug;
            sel[lane] = h;
        }
    }
    __syncthreads();
    copy_parent_rows<W>(a, r0, pl, tid, sel);
}

}  // namespace

extern "C" int svpc_beam_step_groups(const float* scores, int ld, const int* row_c, const int* row_x, int n_sent, int beam, int pos, int logits,
                                     int unk, int eos, int pad, int slot_rows, float* cum, int* finished, const int* text_in,
                                     const int* ext_in, const int* rows_in, int* text_out, int* ext_out, int* rows_out, int ld_tok,
                                     int* parent, int* next_ext, int* next_model, int min_len, int ngram, const unsigned* excl, int excl_v,
                                     const double* lp, int* len, int groups, const float* pen, float* aug, hipStream_t stream) {
    if (n_sent == 0) return 0;
    BEAM_REQUIRE_COMMON("beam_step_groups");
    BEAM_REQUIRE_CTL("beam_step_groups");
    SVPC_REQUIRE(groups >= 1 && beam % groups == 0, "beam_step_groups: the number of groups must divide the beam width");
    SVPC_REQUIRE(len != nullptr && pen != nullptr && aug != nullptr, "beam_step_groups: the length array, the penalty table and aug are required");
    const BeamArgs a = BEAM_COMMON_ARGS;
    const BeamCtl ctl{min_len, ngram, excl, excl_v, lp, len};
    const GroupArgs ga{groups, pen, aug};
    return beam_dispatch("beam_step_groups", beam, [&](auto w) {
        hipLaunchKernelGGL((beam_step_groups_kernel<decltype(w)::value>), dim3(n_sent), dim3(kBeamThreads), 0, stream, a, ctl, ga);
    });
}
