// The skeleton of the beam-search selection kernels (beam.hip: svpc_beam_step / _ctl / _para; beam_groups.hip: svpc_beam_step_groups;
// beam_cons.hip: svpc_beam_step_cons; beam_gumbel.hip: svpc_beam_step_gumbel), written once: the launch shape and the common kernel
// arguments, the parents' values in LDS, a row's top-B columns (one scan under a filter, one shuffle butterfly, lane k's entry k), the
// sentence-scope n-gram bans, a child row's stores, the copy of the parents' token and ancestry rows, the host side's common requirements
// and width dispatch, and the final pick.  A variant keeps what is its own: its candidates' keys, its ranking and its extra state.
#pragma once
#include "common.h"
#include "score_row.h"

#include <climits>
#include <type_traits>

constexpr int kBeamMax = 8;
constexpr int kBeamThreads = 256;

struct BeamArgs {                                  // what every step kernel takes
    const float* scores; int ld; const int* row_c; const int* row_x;
    int pos; int logits; int unk; int eos; int pad; int slot_rows;
    float* cum; int* finished;
    const int* text_in; const int* ext_in; const int* rows_in;
    int* text_out; int* ext_out; int* rows_out; int ld_tok;
    int* parent; int* next_ext; int* next_model;
};

struct BeamCtl {                                   // decoding controls (0 / null: off)
    int min_len; int ngram; const unsigned* excl; int excl_v; const double* lp; int* len;
};

// ---- a row's top-B columns -----------------------------------------------------------------------------------------------------------
// the order of a list: higher key (a raw value, or beam_gumbel.hip's fp64 perturbed log-probability), then lower column
template <class K>
__device__ __forceinline__ bool key_better(K v, int c, K w, int d) { return v > w || (v == w && c < d); }

// insert (v, c) into the sorted top-B list (val, idx); entries past the last real one hold (-inf, INT_MAX)
template <int B, class K>
__device__ __forceinline__ void topb_insert(K (&val)[B], int (&idx)[B], K v, int c) {
    if (!key_better(v, c, val[B - 1], idx[B - 1])) return;
#pragma unroll
    for (int k = 0; k < B; ++k) {
        if (key_better(v, c, val[k], idx[k])) {
            const K tv = val[k]; const int ti = idx[k];
            val[k] = v; idx[k] = c; v = tv; c = ti;
        }
    }
}

// column filters of the scan, asked only about a column that would enter the lane's list
struct NoBan { __device__ __forceinline__ bool operator()(int) const { return false; } };
struct BanList {                                   // ban[0 … nb): a row's banned words, a short LDS list
    const int* ban; int nb;
    __device__ __forceinline__ bool operator()(int c) const {
        for (int k = 0; k < nb; ++k)
            if (ban[k] == c) return true;
        return false;
    }
};

// The top-B of row columns 0 … C − 1 without UNK and skip_eos, called by the 64 lanes of the row's wave: key(c, v) gives column c's key
// v (false: not a candidate), banned(c) filters; every lane scans its columns lane, lane + 64, …, then the lanes merge by a shuffle
// butterfly (lanes l and l^o hold disjoint sets, both end with their merged list): every lane returns with the row's full list.
template <int B, class K, class Key, class Ban>
__device__ __forceinline__ void topb_row(K (&val)[B], int (&idx)[B], int C, int lane, int unk, int skip_eos, Key key, Ban banned) {
#pragma unroll
    for (int k = 0; k < B; ++k) { val[k] = -INFINITY; idx[k] = INT_MAX; }
    for (int c = lane; c < C; c += 64) {
        if (c == unk || c == skip_eos) continue;
        K v;
        if (!key(c, v) || !key_better(v, c, val[B - 1], idx[B - 1]) || banned(c)) continue;
        topb_insert<B>(val, idx, v, c);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        K ov[B]; int oi[B];
#pragma unroll
        for (int k = 0; k < B; ++k) { ov[k] = __shfl_xor(val[k], o, 64); oi[k] = __shfl_xor(idx[k], o, 64); }
#pragma unroll
        for (int k = 0; k < B; ++k) topb_insert<B>(val, idx, ov[k], oi[k]);
    }
}

// the key of a plain row: its raw value
struct RawKey {
    const float* row;
    __device__ __forceinline__ bool operator()(int c, float& v) const { v = row[c]; return true; }
};

// lane k < B keeps entry k of the list every lane holds
template <int B, class K>
__device__ __forceinline__ void topb_entry(const K (&val)[B], const int (&idx)[B], int lane, K& v, int& c) {
    v = val[0]; c = idx[0];
#pragma unroll
    for (int k = 1; k < B; ++k) if (lane == k) { v = val[k]; c = idx[k]; }
}

// ---- prologue ------------------------------------------------------------------------------------------------------------------------
// the parents' values of the sentence whose rows start at r0, read into LDS before any write (len null: 0); the caller's barrier publishes
template <int B>
__device__ __forceinline__ void load_parents(const BeamArgs& a, const int* len, int r0, int tid, float* p_cum, int* p_fin, int* p_len) {
    if (tid < B) { p_cum[tid] = a.cum[r0 + tid]; p_fin[tid] = a.finished[r0 + tid]; p_len[tid] = len ? len[r0 + tid] : 0; }
}

__device__ __forceinline__ bool excluded(const BeamCtl& ctl, int y) {
    return ctl.excl != nullptr && y >= 0 && y < ctl.excl_v && ((ctl.excl[y >> 5] >> (y & 31)) & 1u);
}

// n-gram blocking, sentence scope: the banned words of every live row h of the sentence whose rows start at r0, into ban[h][0 … n_ban[h]).
// Called by the whole workgroup when the step blocks (ctl.ngram > 0, pl >= ctl.ngram); one wave per row, lane l holds y_l, one lane per
// start j = 1 … p − n of an earlier gram.  The caller's barrier publishes the lists.
template <int B>
__device__ __forceinline__ void ngram_ban_rows(const BeamArgs& a, const BeamCtl& ctl, int r0, int pl, int lane, int wave, int (*ban)[64],
                                               int* n_ban) {
    const int n = ctl.ngram, s0 = pl - n + 1;   // the (n − 1)-suffix y_{s0} … y_pos of the new gram
    for (int h = __builtin_amdgcn_readfirstlane(wave); h < B; h += kBeamThreads / 64) {
        if (a.finished[r0 + h]) {             // (wave-uniform; the row's wave is the only writer of n_ban[h] before the barrier)
            if (lane == 0) n_ban[h] = 0;
            continue;
        }
        const int y = lane <= a.pos ? a.ext_in[(size_t)(r0 + h) * a.ld_tok + lane] : -1;
        const bool ex = excluded(ctl, y);
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

// the prologue of a kernel that blocks n-grams at sentence scope: every row's ban list, empty while the step does not block
template <int B>
__device__ __forceinline__ void ngram_bans(const BeamArgs& a, const BeamCtl& ctl, int r0, int pl, int tid, int (*ban)[64], int* n_ban) {
    if (ctl.ngram == 0 || pl < ctl.ngram) {
        if (tid < B) n_ban[tid] = 0;
    } else {
        ngram_ban_rows<B>(a, ctl, r0, pl, tid & 63, tid >> 6, ban, n_ban);
    }
}

// ---- epilogue ------------------------------------------------------------------------------------------------------------------------
// The stores of child row r at position pl = pos + 1: parent row par (of at most max_c columns) picked column col for a summed score cum
// and a length ln.  was_fin: a finished parent carried forward or a fill row (parent the slot itself, cum −inf): its token is PAD.  A
// copied word (one of the row's last X columns) reaches the model as UNK.  The variant's own state is stored beside the call.
__device__ __forceinline__ void write_child(const BeamArgs& a, int* len, int pl, int r, int par, int col, bool was_fin, float cum, int ln,
                                            int max_c = INT_MAX) {
    const int C = min(a.row_c[par], max_c), X = a.row_x[par];
    const int ext = was_fin ? a.pad : col;
    const int mod = was_fin ? a.pad : (col >= C - X ? a.unk : col);
    a.cum[r] = cum;
    a.finished[r] = (was_fin || ext == a.eos) ? 1 : 0;
    if (len) len[r] = ln;
    a.parent[r] = par;
    a.next_ext[r] = ext;
    a.next_model[r] = mod;
    a.text_out[(size_t)r * a.ld_tok + pl] = mod;
    a.ext_out[(size_t)r * a.ld_tok + pl] = ext;
    a.rows_out[(size_t)r * a.ld_tok + pl] = r * a.slot_rows + pl;
}

// tokens of a child: its parent's positions 0 … pos (child k of the sentence has parent r0 + sel[k]), then its own pick at pos + 1
template <int B>
__device__ __forceinline__ void copy_parent_rows(const BeamArgs& a, int r0, int pl, int tid, const int* sel) {
    for (int e = tid; e < B * pl; e += kBeamThreads) {
        const int k = e / pl, j = e - k * pl;
        const size_t src = (size_t)(r0 + sel[k]) * a.ld_tok + j, dst = (size_t)(r0 + k) * a.ld_tok + j;
        a.text_out[dst] = a.text_in[src];
        a.ext_out[dst] = a.ext_in[src];
        a.rows_out[dst] = a.rows_in[src];
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------
// what every step entry point requires (who: its name, a string literal), and what those with svpc_beam_step_ctl's controls add
#define BEAM_REQUIRE_COMMON(who)                                                                                                          \
    SVPC_REQUIRE(beam >= 1 && beam <= kBeamMax, who ": beam width must be 1..8");                                                         \
    SVPC_REQUIRE(pos >= 0 && pos + 1 < ld_tok && pos + 1 < slot_rows, who ": position pos + 1 must lie inside the token / ancestry rows"); \
    SVPC_REQUIRE(text_in != text_out && ext_in != ext_out && rows_in != rows_out, who ": the token and ancestry tables are ping-pong pairs")
#define BEAM_REQUIRE_CTL(who)                                                                                                             \
    SVPC_REQUIRE(min_len >= 0 && min_len < ld_tok && ngram >= 0 && ngram < ld_tok, who ": min length and n-gram size must be 0..ld_tok-1"); \
    SVPC_REQUIRE(ngram == 0 || ld_tok <= 64, who ": n-gram blocking holds a hypothesis's ids in one wave (ld_tok <= 64)");                \
    SVPC_REQUIRE(excl == nullptr || excl_v > 0, who ": the exclusion bitmap needs its id count")

// the common kernel arguments from an entry point's parameters of the same names
#define BEAM_COMMON_ARGS                                                                                                                  \
    BeamArgs{scores, ld, row_c, row_x, pos, logits, unk, eos, pad, slot_rows, cum, finished, text_in, ext_in, rows_in,                    \
             text_out, ext_out, rows_out, ld_tok, parent, next_ext, next_model}

// launch(std::integral_constant<int, W>) with W = beam, one workgroup of kBeamThreads per sentence being the launch's business
template <class Launch>
int beam_dispatch(const char* who, int beam, Launch launch) {
    switch (beam) {
        case 1: launch(std::integral_constant<int, 1>{}); break;
        case 2: launch(std::integral_constant<int, 2>{}); break;
        case 3: launch(std::integral_constant<int, 3>{}); break;
        case 4: launch(std::integral_constant<int, 4>{}); break;
        case 5: launch(std::integral_constant<int, 5>{}); break;
        case 6: launch(std::integral_constant<int, 6>{}); break;
        case 7: launch(std::integral_constant<int, 7>{}); break;
        default: launch(std::integral_constant<int, 8>{}); break;
    }
    return svpc_check_launch(who);
}

// ---- the final pick ------------------------------------------------------------------------------------------------------------------
// per sentence the n_best of its B final hypotheses by the key (double)cum / lp[len] (lp null: cum), ties to the lower beam index: a
// selection by strict comparison from beam 0 up, so n_best = 1 without lp is the first maximum of cum.  CONS (constrained beam search): a
// tier ranks above the key — rows with cum = −inf last, otherwise more constraints met (bits 0–3 of cstate) first — and best_met gets them.
namespace {      // (a kernel of the file that includes this: internal linkage, like its step kernels)

template <bool CONS>
__global__ __launch_bounds__(256) void beam_finalize_kernel(const float* __restrict__ cum, const int* __restrict__ len,
                                                            const double* __restrict__ lp, const int* __restrict__ ext,
                                                            const int* __restrict__ cstate, int ld_tok, int n_sent, int B, int lt,
                                                            int n_best, int* __restrict__ best_ids, float* __restrict__ best_score,
                                                            int* __restrict__ best_len, int* __restrict__ best_met) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_sent) return;
    unsigned taken = 0;
    for (int k = 0; k < n_best; ++k) {
        int hb = -1, tb = 0; double kb = 0.0;      // tb: the tier, 0 for cum = −inf, else 1 + the constraints met
        for (int h = 0; h < B; ++h) {
            if ((taken >> h) & 1u) continue;
            const size_t i = (size_t)t * B + h;
            const double key = lp ? (double)cum[i] / lp[min(max(len[i], 0), ld_tok - 1)] : (double)cum[i];
            int tier = 0;
            if constexpr (CONS) tier = cum[i] == -INFINITY ? 0 : 1 + __popc((unsigned)cstate[i] & 15u);
            if (hb < 0 || tier > tb || (tier == tb && key > kb)) { kb = key; tb = tier; hb = h; }
        }
        taken |= 1u << hb;
        const size_t i = (size_t)t * B + hb, o = (size_t)t * n_best + k;
        best_score[o] = cum[i];
        if constexpr (CONS) best_met[o] = cstate[i] & 15;
        if (best_len) best_len[o] = len ? len[i] : 0;
        const int* src = ext + i * ld_tok;
        for (int j = 0; j < lt; ++j) best_ids[o * lt + j] = src[j];
    }
}

}  // namespace

template <bool CONS>
int beam_finalize(const float* cum, const int* len, const double* lp, const int* ext, const int* cstate, int ld_tok, int n_sent, int beam,
                  int lt, int n_best, int* best_ids, float* best_score, int* best_len, int* best_met, hipStream_t stream) {
#define BEAM_FINALIZE_WHO(msg) (CONS ? "beam_finalize_cons" msg : "beam_finalize" msg)
    if (n_sent == 0) return 0;
    SVPC_REQUIRE(beam >= 1 && beam <= kBeamMax && lt >= 1 && lt <= ld_tok, BEAM_FINALIZE_WHO(": beam width 1..8, 1 <= lt <= ld_tok"));
    SVPC_REQUIRE(n_best >= 1 && n_best <= beam, BEAM_FINALIZE_WHO(": n_best must be 1..beam"));
    SVPC_REQUIRE(lp == nullptr || len != nullptr, BEAM_FINALIZE_WHO(": a length penalty needs the length array"));
    SVPC_REQUIRE(!CONS || (cstate != nullptr && best_met != nullptr), "beam_finalize_cons: cstate and best_met are required");
    hipLaunchKernelGGL(beam_finalize_kernel<CONS>, dim3((n_sent + 255) / 256), dim3(256), 0, stream, cum, len, lp, ext, cstate, ld_tok,
                       n_sent, beam, lt, n_best, best_ids, best_score, best_len, best_met);
    return svpc_check_launch(BEAM_FINALIZE_WHO(""));
#undef BEAM_FINALIZE_WHO
}
