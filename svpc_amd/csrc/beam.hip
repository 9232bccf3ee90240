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

// the same with the banned words as a bitmap (paragraph scope)
template <int B>
__device__ __forceinline__ void topb_insert_bits(float (&val)[B], int (&idx)[B], float v, int c, const unsigned* bits) {
    if (!raw_better(v, c, val[B - 1], idx[B - 1])) return;
    if (c < kBanCols && ((bits[c >> 5] >> (c & 31)) & 1u)) return;
    topb_insert<B>(val, idx, v, c);
}

template <int B, bool PARA>
__global__ __launch_bounds__(kBeamThreads) void beam_step_kernel(BeamArgs a) {
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
    if (tid < B) {
        p_cum[tid] = a.cum[r0 + tid]; p_fin[tid] = a.finished[r0 + tid]; p_len[tid] = a.len ? a.len[r0 + tid] : 0;
    }
    if (tid < NC) c_flat[tid] = INT_MAX;
    if (a.ngram == 0 || pl < a.ngram) {
        if (tid < B) n_ban[tid] = 0;
    } else if constexpr (!PARA) {
        ngram_ban_rows<B>(a, r0, pl, lane, wave, ban, n_ban);
    } else {           // paragraph scope: the row's own pass as above, then one wave-wide pass per earlier sentence, into the bitmap
        const int n = a.ngram, s0 = pl - n + 1;
        const unsigned long long gm = (1ull << n) - 1ull;      // (n <= 63)
        const int h_first = a.hdesc[2 * t], h_count = a.hdesc[2 * t + 1];
        for (int h = __builtin_amdgcn_readfirstlane(wave); h < B; h += kBeamThreads / 64) {
            if (a.finished[r0 + h]) {
                if (lane == 0) n_ban[h] = 0;
                continue;
            }
            unsigned* bits = ban_bits[h];
            const int nw = (min(a.row_c[r0 + h], kBanCols) + 31) >> 5;
            for (int k = lane; k < nw; k += 64) bits[k] = 0u;
            const int y = lane <= a.pos ? a.ext_in[(size_t)(r0 + h) * a.ld_tok + lane] : -1;
            const bool ex = excluded(a, y);
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
                const int z = lane < a.ld_tok ? a.hist[(size_t)(h_first + q) * a.ld_tok + lane] : a.pad;
                const unsigned long long stop = __ballot(lane >= 1 && (z == a.eos || z == a.pad));
                const int last = stop ? __ffsll((long long)stop) - 2 : a.ld_tok - 1;      // the last word position L
                const unsigned long long vm = __ballot(lane >= 1 && lane <= last && z != a.bos);
                match = lane >= 1 && lane + n - 1 <= last && ((vm >> lane) & gm) == gm;
                for (int k = 0; k < n - 1; ++k) match &= __shfl(z, lane + k, 64) == __shfl(y, s0 + k, 64);
                w = __shfl(z, lane + n - 1, 64);
                banned = match && !excluded(a, w);
                nb += __popcll(__ballot(banned));
                if (banned && w >= 0 && w < kBanCols) atomicOr(&bits[w >> 5], 1u << (w & 31));
            }
            if (lane == 0) n_ban[h] = nb;
        }
    }
    __syncthreads();
    const int skip_eos = pl <= a.min_len ? a.eos : a.unk;     // min length: EOS is skipped like UNK
    // one wave per hypothesis row (B > 4: two rows per wave), the rows of a sentence side by side; no barrier inside a row
    for (int h = __builtin_amdgcn_readfirstlane(wave); h < B; h += kBeamThreads / 64) {
        const int r = r0 + h, C = a.row_c[r];
        if (p_fin[h]) {                           // (wave-uniform branch) a finished hypothesis carries itself forward
            if (lane == 0) {
                const int ln = min(max(p_len[h], 0), a.ld_tok - 1);
                c_key[h * B] = a.lp ? (double)p_cum[h] / a.lp[ln] : (double)p_cum[h];
                c_cum[h * B] = p_cum[h]; c_raw[h * B] = INFINITY; c_flat[h * B] = h * C + a.pad; c_par[h * B] = h; c_col[h * B] = a.pad;
            }
            continue;
        }
        const float* row = a.scores + (size_t)r * a.ld;
        const double lse = a.logits ? row_lse(row, C, a.unk, lane) : 0.0;     // log-sum-exp over the row's columns, UNK excluded (fp64)
        float val[B]; int idx[B];
#pragma unroll
        for (int k = 0; k < B; ++k) { val[k] = -INFINITY; idx[k] = INT_MAX; }
        const int nb = n_ban[h];
        if (nb == 0) {
            for (int c = lane; c < C; c += 64)
                if (c != a.unk && c != skip_eos) topb_insert<B>(val, idx, row[c], c);
        } else if constexpr (PARA) {
            for (int c = lane; c < C; c += 64)
                if (c != a.unk && c != skip_eos) topb_insert_bits<B>(val, idx, row[c], c, ban_bits[h]);
        } else {
            for (int c = lane; c < C; c += 64)
                if (c != a.unk && c != skip_eos) topb_insert_ban<B>(val, idx, row[c], c, ban[h], nb);
        }
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
                const float step = step_score(v, a.logits, lse);
                const int e = h * B + lane;
                const float cu = p_cum[h] + step;
                c_key[e] = a.lp ? (double)cu / a.lp[pl] : (double)cu;
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
    // tokens of a child: its parent's positions 0 … pos, then its own pick at pos + 1
    if (tid < B) {
        const int r = r0 + tid;
        int h, col; float cu;
        if (tid < n_cand) { const int e = sel[tid]; h = c_par[e]; col = c_col[e]; cu = c_cum[e]; }
        else { h = tid; col = a.pad; cu = -INFINITY; }     // (fewer than B candidates: a row with < B columns besides UNK, or bans)
        const int C = a.row_c[r0 + h], X = a.row_x[r0 + h];
        const bool was_fin = p_fin[h] != 0 || tid >= n_cand;
        const int ext = was_fin ? a.pad : col;
        const int mod = was_fin ? a.pad : (col >= C - X ? a.unk : col);
        a.cum[r] = cu;
        a.finished[r] = (was_fin || ext == a.eos) ? 1 : 0;
        if (a.len) a.len[r] = (tid < n_cand && p_fin[h]) ? p_len[h] : pl;    // a finished parent keeps its length
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

// per sentence the n_best of its B final hypotheses by the key (double)cum / lp[len] (lp null: cum), ties to the lower beam index: a
// selection by strict comparison from beam 0 up, so n_best = 1 without lp is the first maximum of cum
__global__ __launch_bounds__(256) void beam_finalize_kernel(const float* __restrict__ cum, const int* __restrict__ len,
                                                            const double* __restrict__ lp, const int* __restrict__ ext, int ld_tok,
                                                            int n_sent, int B, int lt, int n_best, int* __restrict__ best_ids,
                                                            float* __restrict__ best_score, int* __restrict__ best_len) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_sent) return;
    unsigned taken = 0;
    for (int k = 0; k < n_best; ++k) {
        int hb = -1; double kb = 0.0;
        for (int h = 0; h < B; ++h) {
            if ((taken >> h) & 1u) continue;
            const size_t i = (size_t)t * B + h;
            const double key = lp ? (double)cum[i] / lp[min(max(len[i], 0), ld_tok - 1)] : (double)cum[i];
            if (hb < 0 || key > kb) { kb = key; hb = h; }
        }
        taken |= 1u << hb;
        const size_t i = (size_t)t * B + hb, o = (size_t)t * n_best + k;
        best_score[o] = cum[i];
        if (best_len) best_len[o] = len ? len[i] : 0;
        const int* src = ext + i * ld_tok;
        for (int j = 0; j < lt; ++j) best_ids[o * lt + j] = src[j];
    }
}

template <bool PARA>
int launch_beam_step(const BeamArgs& a, int n_sent, int beam, hipStream_t stream) {
    const dim3 grid(n_sent), block(kBeamThreads);
    switch (beam) {
        case 1: hipLaunchKernelGGL((beam_step_kernel<1, PARA>), grid, block, 0, stream, a); break;
        case 2: hipLaunchKernelGGL((beam_step_kernel<2, PARA>), grid, block, 0, stream, a); break;
        case 3: hipLaunchKernelGGL((beam_step_kernel<3, PARA>), grid, block, 0, stream, a); break;
        case 4: hipLaunchKernelGGL((beam_step_kernel<4, PARA>), grid, block, 0, stream, a); break;
        case 5: hipLaunchKernelGGL((beam_step_kernel<5, PARA>), grid, block, 0, stream, a); break;
        case 6: hipLaunchKernelGGL((beam_step_kernel<6, PARA>), grid, block, 0, stream, a); break;
        case 7: hipLaunchKernelGGL((beam_step_kernel<7, PARA>), grid, block, 0, stream, a); break;
        default: hipLaunchKernelGGL((beam_step_kernel<8, PARA>), grid, block, 0, stream, a); break;
    }
    return svpc_check_launch("beam_step");
}

}  // namespace

extern "C" {

int svpc_beam_step_ctl(const float* scores, int ld, const int* row_c, const int* row_x, int n_sent, int beam, int pos, int logits, int unk,
                       int eos, int pad, int slot_rows, float* cum, int* finished, const int* text_in, const int* ext_in, const int* rows_in,
                       int* text_out, int* ext_out, int* rows_out, int ld_tok, int* parent, int* next_ext, int* next_model, int min_len,
                       int ngram, const unsigned* excl, int excl_v, const double* lp, int* len, hipStream_t stream) {
    if (n_sent == 0) return 0;
    SVPC_REQUIRE(beam >= 1 && beam <= kBeamMax, "beam_step: beam width must be 1..8");
    SVPC_REQUIRE(pos >= 0 && pos + 1 < ld_tok && pos + 1 < slot_rows, "beam_step: position pos + 1 must lie inside the token / ancestry rows");
    SVPC_REQUIRE(text_in != text_out && ext_in != ext_out && rows_in != rows_out, "beam_step: the token and ancestry tables are ping-pong pairs");
    SVPC_REQUIRE(min_len >= 0 && min_len < ld_tok && ngram >= 0 && ngram < ld_tok, "beam_step: min length and n-gram size must be 0..ld_tok-1");
    SVPC_REQUIRE(ngram == 0 || ld_tok <= 64, "beam_step: n-gram blocking holds a hypothesis's ids in one wave (ld_tok <= 64)");
    SVPC_REQUIRE(lp == nullptr || len != nullptr, "beam_step: a length penalty needs the length array");
    SVPC_REQUIRE(excl == nullptr || excl_v > 0, "beam_step: the exclusion bitmap needs its id count");
    BeamArgs a{scores, ld, row_c, row_x, pos, logits, unk, eos, pad, slot_rows, cum, finished, text_in, ext_in, rows_in,
               text_out, ext_out, rows_out, ld_tok, parent, next_ext, next_model, min_len, ngram, excl, excl_v, lp, len, nullptr, nullptr, 0};
    return launch_beam_step<false>(a, n_sent, beam, stream);
}

int svpc_beam_step_para(const float* scores, int ld, const int* row_c, const int* row_x, int n_sent, int beam, int pos, int logits, int unk,
                        int eos, int pad, int slot_rows, float* cum, int* finished, const int* text_in, const int* ext_in, const int* rows_in,
                        int* text_out, int* ext_out, int* rows_out, int ld_tok, int* parent, int* next_ext, int* next_model, int min_len,
                        int ngram, const unsigned* excl, int excl_v, const double* lp, int* len, const int* hist, const int* hist_desc,
                        int bos, hipStream_t stream) {
    if (n_sent == 0) return 0;
    SVPC_REQUIRE(beam >= 1 && beam <= kBeamMax, "beam_step_para: beam width must be 1..8");
    SVPC_REQUIRE(pos >= 0 && pos + 1 < ld_tok && pos + 1 < slot_rows, "beam_step_para: position pos + 1 must lie inside the token / ancestry rows");
    SVPC_REQUIRE(text_in != text_out && ext_in != ext_out && rows_in != rows_out, "beam_step_para: the token and ancestry tables are ping-pong pairs");
    SVPC_REQUIRE(min_len >= 0 && min_len < ld_tok && ngram >= 1 && ngram < ld_tok, "beam_step_para: min length 0..ld_tok-1, n-gram size 1..ld_tok-1");
    SVPC_REQUIRE(ld_tok <= 64, "beam_step_para: n-gram blocking holds a caption's ids in one wave (ld_tok <= 64)");
    SVPC_REQUIRE(lp == nullptr || len != nullptr, "beam_step_para: a length penalty needs the length array");
    SVPC_REQUIRE(excl == nullptr || excl_v > 0, "beam_step_para: the exclusion bitmap needs its id count");
    SVPC_REQUIRE(hist != nullptr && hist_desc != nullptr, "beam_step_para: the history matrix and its descriptors are required");
    BeamArgs a{scores, ld, row_c, row_x, pos, logits, unk, eos, pad, slot_rows, cum, finished, text_in, ext_in, rows_in,
               text_out, ext_out, rows_out, ld_tok, parent, next_ext, next_model, min_len, ngram, excl, excl_v, lp, len, hist, hist_desc, bos};
    return launch_beam_step<true>(a, n_sent, beam, stream);
}

int svpc_beam_step(const float* scores, int ld, const int* row_c, const int* row_x, int n_sent, int beam, int pos, int logits, int unk,
                   int eos, int pad, int slot_rows, float* cum, int* finished, const int* text_in, const int* ext_in, const int* rows_in,
                   int* text_out, int* ext_out, int* rows_out, int ld_tok, int* parent, int* next_ext, int* next_model,
                   hipStream_t stream) {
    return svpc_beam_step_ctl(scores, ld, row_c, row_x, n_sent, beam, pos, logits, unk, eos, pad, slot_rows, cum, finished, text_in, ext_in,
                              rows_in, text_out, ext_out, rows_out, ld_tok, parent, next_ext, next_model, 0, 0, nullptr, 0, nullptr, nullptr,
                              stream);
}

int svpc_beam_finalize_nbest(const float* cum, const int* len, const double* lp, const int* ext, int ld_tok, int n_sent, int beam, int lt,
                             int n_best, int* best_ids, float* best_score, int* best_len, hipStream_t stream) {
    if (n_sent == 0) return 0;
    SVPC_REQUIRE(beam >= 1 && beam <= kBeamMax && lt >= 1 && lt <= ld_tok, "beam_finalize: beam width 1..8, 1 <= lt <= ld_tok");
    SVPC_REQUIRE(n_best >= 1 && n_best <= beam, "beam_finalize: n_best must be 1..beam");
    SVPC_REQUIRE(lp == nullptr || len != nullptr, "beam_finalize: a length penalty needs the length array");
    hipLaunchKernelGGL(beam_finalize_kernel, dim3((n_sent + 255) / 256), dim3(256), 0, stream, cum, len, lp, ext, ld_tok, n_sent, beam, lt,
                       n_best, best_ids, best_score, best_len);
    return svpc_check_launch("beam_finalize");
}

int svpc_beam_finalize(const float* cum, const int* ext, int ld_tok, int n_sent, int beam, int lt, int* best_ids, float* best_score,
                       hipStream_t stream) {
    return svpc_beam_finalize_nbest(cum, nullptr, nullptr, ext, ld_tok, n_sent, beam, lt, 1, best_ids, best_score, nullptr, stream);
}

}  // extern "C"
