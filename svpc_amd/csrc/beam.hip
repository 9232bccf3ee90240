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
//
// Decoding controls (svpc_beam_step_ctl; all off in svpc_beam_step, which is the same kernel): n-gram blocking bans candidate (h, w) when
// the gram (y_{p-n+1} … y_pos, w) already occurs in h's extended ids y_1 … y_pos and none of its tokens is in the exclusion bitmap; min
// length m skips EOS while p = pos + 1 <= m.  Banned and blocked columns are skipped like UNK but stay in the log-sum-exp of logits mode,
// so a survivor's cum is today's.  A length penalty lp (a float64 table by length, null: none) ranks by key = (double)cum / lp[len], len
// = p for a live parent's child and the stored length for a finished one: every child of one live row has the same len, so the key is
// monotone in the raw value there and the per-row top-B by (raw, column) is unchanged; the B·B survivors rank by (key, raw, flat index).
//
// Paragraph scope (svpc_beam_step_para: the PARA instantiation, a separate kernel): n-gram blocking also bans candidate (h, w) when the gram
// (y_{p-n+1} … y_pos, w) equals an n-gram of the words of an earlier sentence of the same video.  Those sentences' chosen captions are rows
// of the decode's own top-1 extended-id matrix `hist`; sentence t reads rows hdesc[2t] … hdesc[2t] + hdesc[2t + 1] − 1.  The words of a
// history row are its ids at positions 1 … L (L + 1: its first EOS or PAD, else ld_tok − 1), BOS not a word; a gram is n consecutive
// positions that are all words, so none spans two sentences.  Each live row's bans (its own and the history's) are merged into an LDS
// bitmap of kBanCols bits, read only by a column that would enter a lane's top-B.
#include "beam_common.h"

namespace {

constexpr int kBanCols = 4096;                     // paragraph scope: columns of a row's ban bitmap (ops.SAMPLE_COLS_MAX)
constexpr int kBanWords = kBanCols / 32;

struct ParaArgs { const int* hist; const int* hdesc; int bos; };     // paragraph scope (PARA only)

struct BanBits {                                   // a row's banned words as a bitmap (paragraph scope; nb = 0: no bitmap was written)
    const unsigned* bits; int nb;
    __device__ __forceinline__ bool operator()(int c) const { return nb != 0 && c < kBanCols && ((bits[c >> 5] >> (c & 31)) & 1u); }
};

template <int B, bool PARA>
__global__ __launch_bounds__(kBeamThreads) void beam_step_kernel(BeamArgs a, BeamCtl ctl, ParaArgs pa) {
    constexpr int NC = B * B;                      // candidates that reach the final ranking (≤ 64: one lane each)
    __shared__ double c_key[NC];
    __shared__ float c_cum[NC], c_raw[NC];
    __shared__ int c_flat[NC], c_par[NC], c_col[NC];
    __shared__ float p_cum[B];
    __shared__ int p_fin[B], p_len[B], n_cand;
    __shared__ int sel[B];
    __shared__ int ban[PARA ? 1 : B][64], n_ban[B];                         // n-gram blocking: the banned words of every live row
    __shared__ unsigned ban_bits[PARA ? B : 1][PARA ? kBanWords : 1];      // … as a bitmap per row (paragraph scope)
    const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r0 = t * B;
    const int pl = a.pos + 1;                     // position p of this step's pick
    load_parents<B>(a, ctl.len, r0, tid, p_cum, p_fin, p_len);
    if (tid < NC) c_flat[tid] = INT_MAX;
    if constexpr (!PARA) {
        ngram_bans<B>(a, ctl, r0, pl, tid, ban, n_ban);
    } else if (ctl.ngram == 0 || pl < ctl.ngram) {
        if (tid < B) n_ban[tid] = 0;
    } else {           // paragraph scope: the row's own pass as in ngram_ban_rows, then one wave-wide pass per earlier sentence, into the bitmap
        const int n = ctl.ngram, s0 = pl - n + 1;
        const unsigned long long gm = (1ull << n) - 1ull;      // (n <= 63)
        const int h_first = pa.hdesc[2 * t], h_count = pa.hdesc[2 * t + 1];
        for (int h = __builtin_amdgcn_readfirstlane(wave); h < B; h += kBeamThreads / 64) {
            if (a.finished[r0 + h]) {
                if (lane == 0) n_ban[h] = 0;
                continue;
            }
            unsigned* bits = ban_bits[h];
            const int nw = (min(a.row_c[r0 + h], kBanCols) + 31) >> 5;
            for (int k = lane; k < nw; k += 64) bits[k] = 0u;
            const int y = lane <= a.pos ? a.ext_in[(size_t)(r0 + h) * a.ld_tok + lane] : -1;
            const bool ex = excluded(ctl, y);
            if (__ballot(ex && lane >= s0 && lane <= a.pos) != 0ull) {      // an excluded token in the suffix saves every gram
                if (lane == 0) n_ban[h] = 0;
                continue;
            }
            bool match = lane >= 1 && lane <= pl - n;
            for (int k = 0; k < n - 1; ++k) match &= __shfl(y, lane + k, 64) == __shfl(y, s0 + k, 64);
            int w = __shfl(y, lane + n - 1, 64);
            const bool w_ex = __shfl((int)ex, lane + n - 1, 64) != 0;      // (every lane shuffles: a source lane must be active)
            bool banned = match && !w_ex;
            int nb = __popcll(__ballot(banned));
            if (banned && w >= 0 && w < kBanCols) atomicOr(&bits[w >> 5], 1u << (w & 31));
            for (int q = 0; q < h_count; ++q) {   // lane j holds z_j of the earlier sentence's caption
                const int z = lane < a.ld_tok ? pa.hist[(size_t)(h_first + q) * a.ld_tok + lane] : a.pad;
                const unsigned long long stop = __ballot(lane >= 1 && (z == a.eos || z == a.pad));
                const int last = stop ? __ffsll((long long)stop) - 2 : a.ld_tok - 1;      // the last word position L
                const unsigned long long vm = __ballot(lane >= 1 && lane <= last && z != pa.bos);
                match = lane >= 1 && lane + n - 1 <= last && ((vm >> lane) & gm) == gm;
                for (int k = 0; k < n - 1; ++k) match &= __shfl(z, lane + k, 64) == __shfl(y, s0 + k, 64);
                w = __shfl(z, lane + n - 1, 64);
                banned = match && !excluded(ctl, w);
                nb += __popcll(__ballot(banned));
                if (banned && w >= 0 && w < kBanCols) atomicOr(&bits[w >> 5], 1u << (w & 31));
            }
            if (lane == 0) n_ban[h] = nb;
        }
    }
    __syncthreads();
    const int skip_eos = pl <= ctl.min_len ? a.eos : a.unk;   // min length: EOS is skipped like UNK
    // one wave per hypothesis row (B > 4: two rows per wave), the rows of a sentence side by side; no barrier inside a row
    for (int h = __builtin_amdgcn_readfirstlane(wave); h < B; h += kBeamThreads / 64) {
        const int r = r0 + h, C = a.row_c[r];
        if (p_fin[h]) {                           // (wave-uniform branch) a finished hypothesis carries itself forward
            if (lane == 0) {
                const int ln = min(max(p_len[h], 0), a.ld_tok - 1);
                c_key[h * B] = ctl.lp ? (double)p_cum[h] / ctl.lp[ln] : (double)p_cum[h];
                c_cum[h * B] = p_cum[h]; c_raw[h * B] = INFINITY; c_flat[h * B] = h * C + a.pad; c_par[h * B] = h; c_col[h * B] = a.pad;
            }
            continue;
        }
        const float* row = a.scores + (size_t)r * a.ld;
        const double lse = a.logits ? row_lse(row, C, a.unk, lane) : 0.0;     // log-sum-exp over the row's columns, UNK excluded (fp64)
        float val[B]; int idx[B];
        if constexpr (PARA) topb_row<B>(val, idx, C, lane, a.unk, skip_eos, RawKey{row}, BanBits{ban_bits[h], n_ban[h]});
        else topb_row<B>(val, idx, C, lane, a.unk, skip_eos, RawKey{row}, BanList{ban[h], n_ban[h]});
        if (lane < B) {
            float v; int c;
            topb_entry<B>(val, idx, lane, v, c);
            if (c != INT_MAX) {
                const float step = step_score(v, a.logits, lse);
                const int e = h * B + lane;
                const float cu = p_cum[h] + step;
                c_key[e] = ctl.lp ? (double)cu / ctl.lp[pl] : (double)cu;
                c_cum[e] = cu; c_raw[e] = v; c_flat[e] = h * C + c; c_par[e] = h; c_col[e] = c;
            }
        }
    }
    __syncthreads();
    if (tid < 64) {                               // rank every candidate against all others: the B best take slots 0 … B-1
        int rank = INT_MAX, n = 0;
        if (tid < NC && c_flat[tid] != INT_MAX) {
            const double ck = c_key[tid]; const float cr = c_raw[tid]; const int cf = c_flat[tid];
            rank = 0;
            for (int j = 0; j < NC; ++j) {
                if (c_flat[j] == INT_MAX) continue;
                const double ok = c_key[j]; const float orw = c_raw[j]; const int of = c_flat[j];
                rank += (ok > ck || (ok == ck && (orw > cr || (orw == cr && of < cf)))) ? 1 : 0;
            }
        }
        if (rank < B) sel[rank] = tid;
        n = __popcll(__ballot(tid < NC && c_flat[tid] != INT_MAX));
        if (tid == 0) n_cand = n;
    }
    __syncthreads();
    if (tid < B) {
        int h, col; float cu;
        if (tid < n_cand) { const int e = sel[tid]; h = c_par[e]; col = c_col[e]; cu = c_cum[e]; }
        else { h = tid; col = a.pad; cu = -INFINITY; }     // (fewer than B candidates: a row with < B columns besides UNK, or bans)
        const bool kept = tid < n_cand && p_fin[h];       // a finished parent keeps its length
        write_child(a, ctl.len, pl, r0 + tid, r0 + h, col, p_fin[h] != 0 || tid >= n_cand, cu, kept ? p_len[h] : pl);
        sel[tid] = h;                             // (read below only after the barrier; every writer has read its entry)
    }
    __syncthreads();
    copy_parent_rows<B>(a, r0, pl, tid, sel);
}

}  // namespace

extern "C" {

int svpc_beam_finalize_nbest(const float* cum, const int* len, const double* lp, const int* ext, int ld_tok, int n_sent, int beam, int lt,
                             int n_best, int* best_ids, float* best_score, int* best_len, hipStream_t stream) {
    return beam_finalize<false>(cum, len, lp, ext, nullptr, ld_tok, n_sent, beam, lt, n_best, best_ids, best_score, best_len, nullptr, stream);
}

int svpc_beam_finalize(const float* cum, const int* ext, int ld_tok, int n_sent, int beam, int lt, int* best_ids, float* best_score,
                       hipStream_t stream) {
    return svpc_beam_finalize_nbest(cum, nullptr, nullptr, ext, ld_tok, n_sent, beam, lt, 1, best_ids, best_score, nullptr, stream);
}

int svpc_beam_step_ctl(const float* scores, int ld, const int* row_c, const int* row_x, int n_sent, int beam, int pos, int logits, int unk,
                       int eos, int pad, int slot_rows, float* cum, int* finished, const int* text_in, const int* ext_in, const int* rows_in,
                       int* text_out, int* ext_out, int* rows_out, int ld_tok, int* parent, int* next_ext, int* next_model, int min_len,
                       int ngram, const unsigned* excl, int excl_v, const double* lp, int* len, hipStream_t stream) {
    if (n_sent == 0) return 0;
    BEAM_REQUIRE_COMMON("beam_step");
    BEAM_REQUIRE_CTL("beam_step");
    SVPC_REQUIRE(lp == nullptr || len != nullptr, "beam_step: a length penalty needs the length array");
    const BeamArgs a = BEAM_COMMON_ARGS;
    const BeamCtl ctl{min_len, ngram, excl, excl_v, lp, len};
    return beam_dispatch("beam_step", beam, [&](auto w) {
        hipLaunchKernelGGL((beam_step_kernel<decltype(w)::value, false>), dim3(n_sent), dim3(kBeamThreads), 0, stream, a, ctl, ParaArgs{});
    });
}

int svpc_beam_step_para(const float* scores, int ld, const int* row_c, const int* row_x, int n_sent, int beam, int pos, int logits, int unk,
                        int eos, int pad, int slot_rows, float* cum, int* finished, const int* text_in, const int* ext_in, const int* rows_in,
                        int* text_out, int* ext_out, int* rows_out, int ld_tok, int* parent, int* next_ext, int* next_model, int min_len,
                        int ngram, const unsigned* excl, int excl_v, const double* lp, int* len, const int* hist, const int* hist_desc,
                        int bos, hipStream_t stream) {
    if (n_sent == 0) return 0;
    BEAM_REQUIRE_COMMON("beam_step_para");
    SVPC_REQUIRE(min_len >= 0 && min_len < ld_tok && ngram >= 1 && ngram < ld_tok, "beam_step_para: min length 0..ld_tok-1, n-gram size 1..ld_tok-1");
    SVPC_REQUIRE(ld_tok <= 64, "beam_step_para: n-gram blocking holds a caption's ids in one wave (ld_tok <= 64)");
    SVPC_REQUIRE(lp == nullptr || len != nullptr, "beam_step_para: a length penalty needs the length array");
    SVPC_REQUIRE(excl == nullptr || excl_v > 0, "beam_step_para: the exclusion bitmap needs its id count");
    SVPC_REQUIRE(hist != nullptr && hist_desc != nullptr, "beam_step_para: the history matrix and its descriptors are required");
    const BeamArgs a = BEAM_COMMON_ARGS;
    const BeamCtl ctl{min_len, ngram, excl, excl_v, lp, len};
    const ParaArgs pa{hist, hist_desc, bos};
    return beam_dispatch("beam_step", beam, [&](auto w) {
        hipLaunchKernelGGL((beam_step_kernel<decltype(w)::value, true>), dim3(n_sent), dim3(kBeamThreads), 0, stream, a, ctl, pa);
    });
}

int svpc_beam_step(const float* scores, int ld, const int* row_c, const int* row_x, int n_sent, int beam, int pos, int logits, int unk,
                   int eos, int pad, int slot_rows, float* cum, int* finished, const int* text_in, const int* ext_in, const int* rows_in,
                   int* text_out, int* ext_out, int* rows_out, int ld_tok, int* parent, int* next_ext, int* next_model,
                   hipStream_t stream) {
    return svpc_beam_step_ctl(scores, ld, row_c, row_x, n_sent, beam, pos, logits, unk, eos, pad, slot_rows, cum, finished, text_in, ext_in,
                              rows_in, text_out, ext_out, rows_out, ld_tok, parent, next_ext, next_model, 0, 0, nullptr, 0, nullptr, nullptr,
                              stream);
}

}  // extern "C"
