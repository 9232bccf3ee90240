// Lexically constrained beam search: the selection step and the final pick (Post & Vilar 2018, "Fast Lexically Constrained Decoding with
// Dynamic Beam Allocation", arXiv 1804.06609; fairseq's --constraints, unordered).  A sentence has M ≤ 4 constraints, each a phrase of 1 … 4
// extended ids: `cons` is (n_sent, 4, 4) int32, a phrase the leading non-negative ids of its row, the constraints of a sentence its leading
// non-empty rows.  Every hypothesis row carries one int32 tracker state (cstate, updated in place like cum): bits 0–3 `met` (one bit per
// constraint met), bits 4–6 cur + 1 (0: no phrase in progress), bits 8–10 `off` (tokens of phrase cur matched so far).  On a picked word c
// of an unfinished parent: cur ≥ 0 and c = phrase[cur][off] → off += 1, and a complete phrase sets its bit and clears (cur, off); otherwise
// the progress is dropped and the lowest unmet phrase whose first id is c starts (or, of length 1, is met).  A finished parent keeps its
// state, a fill row gets 0.  n(state) = Σ_{j met} len[j] + off is the hypothesis's bank.  The tracker is not a string matcher: with phrase
// `a a b` the text `a a a b` does not complete it.  Restated by tests/constrained_beam_reference.py.
//
// Candidates of an unfinished parent h: svpc_beam_step_ctl's allowed columns, EOS also skipped while met(h) is not the full mask; of those
// (a) the row's top-W by (raw, column) — beam_common.h's topb_row, which leaves the list in every lane — and (b) its forced columns:
// phrase[cur][off] if a phrase is in progress, else the first ids of all unmet phrases, each only if allowed and its child's cum' > −inf.
// A column in both is one candidate.
// A finished parent offers itself (PAD, cum and len kept, raw +inf).  Allocation (fairseq's stride over banks): live candidates (cum'
// finite) rank inside their bank by svpc_beam_step_ctl's order (higher key, higher raw value, lower flat index h·C + c); the output order
// is ascending (rank in bank, −bank); dead candidates follow in svpc_beam_step_ctl's total order; the first W become rows 0 … W − 1, missing
// ones are fill rows.  With M = 0 every candidate is in bank 0 and the step is svpc_beam_step_ctl's, bit for bit.
//
// Phase one: one wave per row, register top-W, shuffle butterflies; then lanes W … W + 3 of the row's wave evaluate its ≤ 4 forced columns
// (range, UNK, EOS and ban-list tests, the duplicate test against the top-W every lane holds, the step score through score_row.h): ≤ W + 4
// survivors per row, ≤ 96 per sentence, in LDS.  Phase two: one thread per survivor — child state, bank, key; rank in bank; output
// position — two counting passes over the ≤ 96 LDS entries with a barrier between them; the W winners write their rows.  Phase three copies
// the parents' token and ancestry rows.
#include "beam_common.h"

namespace {

constexpr int kConsMax = 4;                        // constraints of a sentence (ops.CONS_MAX)
constexpr int kConsLen = 4;                        // ids of a phrase (ops.CONS_LEN)

struct ConsArgs { const int* cons; int* cstate; };

struct Track { int met, cur, off; };

// (a state the step did not write itself is taken apart defensively: a phrase index or an offset outside the table means no progress)
__device__ __forceinline__ Track unpack_state(int st, const int* plen, int M) {
    Track k{st & 15, ((st >> 4) & 7) - 1, (st >> 8) & 7};
    if (k.cur >= M || (k.cur >= 0 && k.off >= plen[k.cur])) { k.cur = -1; k.off = 0; }
    if (k.cur < 0) k.off = 0;
    return k;
}

__device__ __forceinline__ int pack_state(const Track& k) { return k.met | ((k.cur + 1) << 4) | (k.off << 8); }

// the tracker: the state of the child that picks the word c
__device__ __forceinline__ int track_word(int st, int c, const int* ph, const int* plen, int M) {
    Track k = unpack_state(st, plen, M);
    if (k.cur >= 0 && c == ph[k.cur * kConsLen + k.off]) {
        k.off += 1;
        if (k.off == plen[k.cur]) { k.met |= 1 << k.cur; k.cur = -1; k.off = 0; }
    } else {
        k.cur = -1; k.off = 0;
        int j = -1;
        for (int q = M - 1; q >= 0; --q)
            if (!((k.met >> q) & 1) && ph[q * kConsLen] == c) j = q;
        if (j >= 0) {
            if (plen[j] == 1) k.met |= 1 << j;
            else { k.cur = j; k.off = 1; }
        }
    }
    return pack_state(k);
}

// n(state): the constraint tokens a hypothesis has banked
__device__ __forceinline__ int bank_of(int st, const int* plen, int M) {
    const Track k = unpack_state(st, plen, M);
    int n = k.off;
    for (int q = 0; q < M; ++q) n += ((k.met >> q) & 1) ? plen[q] : 0;
    return n;
}

// today's strict order of two candidates: higher key, then higher raw value, then lower flat index
__device__ __forceinline__ bool cand_before(double ok, float orw, int of, double key, float raw, int flat) {
    return ok > key || (ok == key && (orw > raw || (orw == raw && of < flat)));
}

template <int W>
__global__ __launch_bounds__(kBeamThreads) void beam_step_cons_kernel(BeamArgs a, BeamCtl ctl, ConsArgs ca) {
    constexpr int NS = W + kConsMax;               // survivors of a row: its top-W columns and its forced columns
    constexpr int NC = W * NS;                     // … of a sentence (≤ 96)
    constexpr int kDead = -1, kNone = -2;          // c_bank of a dead candidate / of an empty entry
    __shared__ double c_key[NC];
    __shared__ float c_step[NC], c_raw[NC];
    __shared__ int c_flat[NC], c_col[NC], c_bank[NC], c_rank[NC];
    __shared__ float p_cum[W];
    __shared__ int p_fin[W], p_len[W], p_st[W];
    __shared__ int ph[kConsMax * kConsLen], plen[kConsMax];
    __shared__ int sel[W];
    __shared__ int ban[W][64], n_ban[W];           // n-gram blocking: the banned words of every live row
    const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r0 = t * W;
    const int pl = a.pos + 1;                      // position p of this step's pick
    load_parents<W>(a, ctl.len, r0, tid, p_cum, p_fin, p_len);
    if (tid < W) p_st[tid] = ca.cstate[r0 + tid];
    if (tid >= 64 && tid < 64 + kConsMax * kConsLen) ph[tid - 64] = ca.cons[(size_t)t * (kConsMax * kConsLen) + tid - 64];
    if (tid >= 128 && tid < 128 + kConsMax) {      // a phrase: the leading non-negative ids of its row
        const int* q = ca.cons + (size_t)t * (kConsMax * kConsLen) + (tid - 128) * kConsLen;
        int n = 0;
        while (n < kConsLen && q[n] >= 0) ++n;
        plen[tid - 128] = n;
    }
    for (int e = tid; e < NC; e += kBeamThreads) c_flat[e] = INT_MAX;
    ngram_bans<W>(a, ctl, r0, pl, tid, ban, n_ban);
    __syncthreads();
    int M = 0;                                     // the constraints of the sentence: its leading non-empty rows
    while (M < kConsMax && plen[M] > 0) ++M;
    const int full = (1 << M) - 1;
    // phase one: one wave per hypothesis row, its top-W columns by (raw, column), its forced columns, and their step scores
    for (int h = __builtin_amdgcn_readfirstlane(wave); h < W; h += kBeamThreads / 64) {
        const int r = r0 + h, C = a.row_c[r];
        if (p_fin[h]) {                            // (wave-uniform branch) a finished hypothesis carries itself forward
            if (lane == 0) { c_step[h * NS] = 0.f; c_raw[h * NS] = INFINITY; c_flat[h * NS] = h * C + a.pad; c_col[h * NS] = a.pad; }
            continue;
        }
        const Track k = unpack_state(p_st[h], plen, M);
        const int skip_eos = (pl <= ctl.min_len || k.met != full) ? a.eos : a.unk;     // EOS is skipped like UNK: min length, unmet constraints
        const float* row = a.scores + (size_t)r * a.ld;
        const double lse = a.logits ? row_lse(row, C, a.unk, lane) : 0.0;
        float val[W]; int idx[W];
        const int nb = n_ban[h];
        topb_row<W>(val, idx, C, lane, a.unk, skip_eos, RawKey{row}, BanList{ban[h], nb});
        if (lane < W) {
            float v; int c;
            topb_entry<W>(val, idx, lane, v, c);
            if (c != INT_MAX) {
                const int e = h * NS + lane;
                c_step[e] = step_score(v, a.logits, lse); c_raw[e] = v; c_flat[e] = h * C + c; c_col[e] = c;
            }
        } else if (lane < NS) {                    // lanes W … W + 3: the row's forced columns
            const int f = lane - W;
            int fc = -1;
            if (k.cur >= 0) {
                if (f == 0) fc = ph[k.cur * kConsLen + k.off];
            } else if (f < M && !((k.met >> f) & 1)) {
                fc = ph[f * kConsLen];
                for (int q = 0; q < f; ++q)        // two unmet phrases with one first id force one column
                    if (!((k.met >> q) & 1) && ph[q * kConsLen] == fc) fc = -1;
            }
            bool ok = fc >= 0 && fc < C && fc != a.unk && fc != skip_eos;
            for (int q = 0; q < nb; ++q) ok = ok && ban[h][q] != fc;
#pragma unroll
            for (int q = 0; q < W; ++q) ok = ok && idx[q] != fc;      // already among the top-W: one candidate
            if (ok) {
                const float v = row[fc];
                const float st = step_score(v, a.logits, lse);
                if (p_cum[h] + st > -INFINITY) {   // (a forced column counts only with a live child)
                    const int e = h * NS + lane;
                    c_step[e] = st; c_raw[e] = v; c_flat[e] = h * C + fc; c_col[e] = fc;
                }
            }
        }
    }
    __syncthreads();
    // phase two: one thread per survivor
    const int e = tid;
    const bool valid = e < NC && c_flat[e] != INT_MAX;
    const int h = valid ? e / NS : 0;
    const bool fin = valid && p_fin[h] != 0;
    int col = a.pad, state = 0, bank = kNone, flat = INT_MAX;
    float cu = -INFINITY, raw = -INFINITY;
    double key = -INFINITY;
    if (valid) {
        flat = c_flat[e]; col = c_col[e];
        if (fin) {
            const int ln = min(max(p_len[h], 0), a.ld_tok - 1);
            cu = p_cum[h]; raw = INFINITY; state = p_st[h];
            key = ctl.lp ? (double)cu / ctl.lp[ln] : (double)cu;
        } else {
            cu = p_cum[h] + c_step[e]; raw = c_raw[e]; state = track_word(p_st[h], col, ph, plen, M);
            key = ctl.lp ? (double)cu / ctl.lp[pl] : (double)cu;
        }
        bank = (cu > -INFINITY && cu < INFINITY) ? bank_of(state, plen, M) : kDead;
    }
    if (e < NC) { c_key[e] = key; c_bank[e] = bank; }
    __syncthreads();
    int rank = 0, n_live = 0, n_cand = 0;          // first pass: the rank inside the bank (a dead candidate: among the dead)
    if (tid < 64 || valid) {                       // (tid < W fills the rows without a candidate: it needs n_cand)
        for (int j = 0; j < NC; ++j) {
            const int ob = c_bank[j];
            if (ob == kNone) continue;
            n_cand += 1;
            n_live += ob != kDead ? 1 : 0;
            rank += (ob == bank && cand_before(c_key[j], c_raw[j], c_flat[j], key, raw, flat)) ? 1 : 0;
        }
    }
    if (e < NC) c_rank[e] = rank;
    __syncthreads();
    int out = INT_MAX;                             // second pass: the output position, ascending (rank in bank, −bank); the dead last
    if (valid) {
        if (bank == kDead) {
            out = n_live + rank;
        } else {
            out = 0;
            for (int j = 0; j < NC; ++j) {
                const int ob = c_bank[j], orank = c_rank[j];
                out += (ob >= 0 && (orank < rank || (orank == rank && ob > bank))) ? 1 : 0;
            }
        }
    }
    if (out < W) {
        write_child(a, ctl.len, pl, r0 + out, r0 + h, col, fin, cu, fin ? p_len[h] : pl);     // (a finished parent keeps its length)
        ca.cstate[r0 + out] = state;
        sel[out] = h;
    }
    if (tid < W && tid >= n_cand) {                // fewer than W candidates: fill rows, as in beam_step_kernel
        write_child(a, ctl.len, pl, r0 + tid, r0 + tid, a.pad, true, -INFINITY, pl);
        ca.cstate[r0 + tid] = 0;
        sel[tid] = tid;
    }
    __syncthreads();
    copy_parent_rows<W>(a, r0, pl, tid, sel);
}

}  // namespace

extern "C" int svpc_beam_finalize_cons(const float* cum, const int* len, const double* lp, const int* ext, const int* cstate, int ld_tok,
                                       int n_sent, int beam, int lt, int n_best, int* best_ids, float* best_score, int* best_len,
                                       int* best_met, hipStream_t stream) {
    return beam_finalize<true>(cum, len, lp, ext, cstate, ld_tok, n_sent, beam, lt, n_best, best_ids, best_score, best_len, best_met, stream);
}

extern "C" int svpc_beam_step_cons(const float* scores, int ld, const int* row_c, const int* row_x, int n_sent, int beam, int pos, int logits,
                                   int unk, int eos, int pad, int slot_rows, float* cum, int* finished, const int* text_in,
                                   const int* ext_in, const int* rows_in, int* text_out, int* ext_out, int* rows_out, int ld_tok,
                                   int* parent, int* next_ext, int* next_model, int min_len, int ngram, const unsigned* excl, int excl_v,
                                   const double* lp, int* len, const int* cons, int* cstate, hipStream_t stream) {
    if (n_sent == 0) return 0;
    BEAM_REQUIRE_COMMON("beam_step_cons");
    BEAM_REQUIRE_CTL("beam_step_cons");
    SVPC_REQUIRE(len != nullptr && cons != nullptr && cstate != nullptr, "beam_step_cons: the length array, the constraint table and cstate are required");
    const BeamArgs a = BEAM_COMMON_ARGS;
    const BeamCtl ctl{min_len, ngram, excl, excl_v, lp, len};
    const ConsArgs ca{cons, cstate};
    return beam_dispatch("beam_step_cons", beam, [&](auto w) {
        hipLaunchKernelGGL((beam_step_cons_kernel<decltype(w)::value>), dim3(n_sent), dim3(kBeamThreads), 0, stream, a, ctl, ca);
    });
}
