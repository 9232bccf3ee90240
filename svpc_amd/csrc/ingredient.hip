// Ingredient-prediction recall / precision / F1 of decoded captions, on the device.
//
// reference: src/calculate_ingredient_f1.py:6-30 (extract_ingredients: `ingredient in sentence`, a substring test, for the recipe's listed
// ingredients; then `word in all_ingredient_dict` for every word that is no whole listed ingredient), :32-59 (calculate_ingredient_f1:
// correct / recall / precision totals over the zip of generated and ground-truth steps).  The reference reads the captions back from the
// JSON that run_translate writes (one device→host copy per sentence, translate.py:81-82).
//
// The string rule is carried by bit tables the host compiles once (svpc_amd/ingredients.py): a listed ingredient is a run
// of pattern tokens, each a predicate on one word (contains / ends with / equals / starts with a string); a predicate is a row of a
// (P, ⌈V/32⌉) bitmap over the vocabulary plus 128 bits over the video's copied words.  Restated by tests/ingredient_f1_reference.py.
//   caption_ingredients_kernel   one wave per clean caption (Lt ≤ 64, one lane per position): per pattern token the lanes fetch their
//                                word's predicate bit, a ballot gives the token's position mask; ingredient e is mentioned when
//                                B[t0] & (B[t0+1] >> 1) & … is not 0 (the ballots are masked by the caption's length, so a pattern
//                                cannot run past the last word); extra words and the hits in the ground-truth step by the same ballots;
//   ingredient_totals_kernel     one workgroup: a thread sums its videos' rows (integers) → the (N, 3) per-video counts and three
//                                64-bit integer atomics into the accumulator (no float: any order gives the same bits).
#include "common.h"

namespace {

constexpr int kRowThreads = 256;              // four captions per workgroup
constexpr int kTotThreads = 256;
constexpr int kVidCols = 8;                   // ing0, E, X, eq0, n_eq, gt0, n_gt, (unused)
constexpr int kCapIngredients = 64;
constexpr int kCapCopied = 128;

struct IngrArgs {
    const int* words; const int* len; int n_rows; int lt;
    const int* row_vs; int n_vid;
    const unsigned* pred; int pred_ld; int n_pred; const unsigned* a_bits; int vocab;
    const int* vid; const int* ing_tok; const int* tok_row; const unsigned* tok_oov; const int* eq_ids; const unsigned* oov_a;
    const unsigned* gt_mask; const int* gt_len; const int* gx_off; const int* gx_ids;
    long long* masks; int* extra; int* row_counts;
};

__global__ __launch_bounds__(kRowThreads) void caption_ingredients_kernel(IngrArgs a) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * (kRowThreads / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (r >= a.n_rows) return;                    // (wave-uniform)
    const int b = a.row_vs[2 * r], s = a.row_vs[2 * r + 1];
    const int* vd = a.vid + (size_t)b * kVidCols;
    const int ing0 = vd[0], E = min(vd[1], kCapIngredients), X = min(vd[2], kCapCopied), eq0 = vd[3], n_eq = vd[4], gt0 = vd[5], n_gt = vd[6];
    const int n = min(max(a.len[r], 0), min(a.lt, 64));
    const bool live = lane < n;
    const int w = live ? a.words[(size_t)r * a.lt + lane] : -1;
    const bool in_v = live && w >= 0 && w < a.vocab;              // a vocabulary word: bit w of a table row
    const int x = w - a.vocab;
    const bool in_x = live && x >= 0 && x < X;                    // a copied word of this video: bit x of the video's 128
    const int wq = in_v ? (w >> 5) : (in_x ? (x >> 5) : 0), wb = (in_v ? w : x) & 31;
    // 1. listed ingredients: the position mask of every pattern token, shifted to the pattern's first position
    u64 mask = 0ull;
    for (int e = 0; e < E; ++e) {
        const int t0 = a.ing_tok[ing0 + e], t1 = a.ing_tok[ing0 + e + 1];
        u64 m = t1 > t0 ? ~0ull : 0ull;
        for (int j = t0; j < t1 && m; ++j) {                      // (m is wave-uniform)
            const int row = a.tok_row[j];
            unsigned bits = 0u;
            if (in_v && row >= 0 && row < a.n_pred) bits = a.pred[(size_t)row * a.pred_ld + wq];
            else if (in_x) bits = a.tok_oov[(size_t)j * (kCapCopied / 32) + wq];
            const u64 hit = __ballot((bits >> wb) & 1u);
            const int sh = j - t0;
            m &= sh < 64 ? hit >> sh : 0ull;
        }
        if (m) mask |= 1ull << e;
    }
    // 2. extra words: no whole listed ingredient, and in the global set A
    bool listed = false;
    for (int i = 0; i < n_eq; ++i) listed |= w == a.eq_ids[eq0 + i];
    unsigned abits = 0u;
    if (in_v) abits = a.a_bits[wq];
    else if (in_x) abits = a.oov_a[(size_t)b * (kCapCopied / 32) + wq];
    const bool is_extra = (in_v || in_x) && !listed && ((abits >> wb) & 1u);
    const int n_extra = __popcll(__ballot(is_extra));
    // 3. against the ground-truth step (the zip: generated step s counts when the video has a ground-truth step s)
    int correct = 0, n_gen = 0, n_ref = 0;
    if (s < n_gt) {                               // (wave-uniform)
        const int g = gt0 + s;
        const u64 gm = (u64)a.gt_mask[2 * g] | ((u64)a.gt_mask[2 * g + 1] << 32);
        bool in_gt = false;
        for (int i = a.gx_off[g]; i < a.gx_off[g + 1]; ++i) in_gt |= w == a.gx_ids[i];
        correct = __popcll(mask & gm) + __popcll(__ballot(is_extra && in_gt));
        n_gen = __popcll(mask) + n_extra;
        n_ref = a.gt_len[g];
    }
    if (lane == 0) {
        a.masks[r] = (long long)mask;
        a.extra[r] = n_extra;
        int* rc = a.row_counts + (size_t)r * 3;
        rc[0] = correct; rc[1] = n_gen; rc[2] = n_ref;
    }
}

__global__ __launch_bounds__(kTotThreads) void ingredient_totals_kernel(const int* __restrict__ row_counts, const int* __restrict__ vid_off,
                                                                        int n_vid, int n_rows, int* __restrict__ vid_counts, u64* acc) {
    __shared__ u64 tot[3];
    const int tid = threadIdx.x;
    if (tid < 3) tot[tid] = 0ull;
    __syncthreads();
    u64 c0 = 0ull, c1 = 0ull, c2 = 0ull;
    for (int b = tid; b < n_vid; b += kTotThreads) {
        const int r0 = max(vid_off[b], 0), r1 = min(vid_off[b + 1], n_rows);
        int v0 = 0, v1 = 0, v2 = 0;
        for (int r = r0; r < r1; ++r) { v0 += row_counts[3 * r]; v1 += row_counts[3 * r + 1]; v2 += row_counts[3 * r + 2]; }
        int* out = vid_counts + (size_t)b * 3;
        out[0] = v0; out[1] = v1; out[2] = v2;
        c0 += (u64)v0; c1 += (u64)v1; c2 += (u64)v2;
    }
    if (c0) atomicAdd(&tot[0], c0);
    if (c1) atomicAdd(&tot[1], c1);
    if (c2) atomicAdd(&tot[2], c2);
    __syncthreads();
    if (acc && tid < 3 && tot[tid]) atomicAdd(acc + tid, tot[tid]);
}

}  // namespace

extern "C" {

int svpc_caption_ingredients(const int* words, const int* len, int n_rows, int lt, const int* vid_off, const int* row_vs, int n_vid,
                             const unsigned* pred, int pred_ld, int n_pred, const unsigned* a_bits, int vocab, const int* vid,
                             const int* ing_tok, const int* tok_row, const unsigned* tok_oov, const int* eq_ids, const unsigned* oov_a,
                             const unsigned* gt_mask, const int* gt_len, const int* gx_off, const int* gx_ids, long long* masks, int* extra,
                             int* row_counts, int* vid_counts, unsigned long long* acc, hipStream_t stream) {
    if (n_rows == 0 && n_vid == 0) return 0;
    SVPC_REQUIRE(lt >= 1 && lt <= 64, "caption_ingredients: rows of 1..64 positions (one lane per position)");
    SVPC_REQUIRE(n_rows >= 0 && n_vid > 0 && vocab >= 1 && pred_ld * 32 >= vocab && n_pred >= 0, "caption_ingredients: sizes out of range");
    SVPC_REQUIRE(words && len && vid_off && row_vs && pred && a_bits && vid && ing_tok && tok_row && tok_oov && eq_ids && oov_a && gt_mask &&
                 gt_len && gx_off && gx_ids && masks && extra && row_counts && vid_counts, "caption_ingredients: buffers are required");
    if (n_rows > 0) {
        IngrArgs a{words, len, n_rows, lt, row_vs, n_vid, pred, pred_ld, n_pred, a_bits, vocab, vid, ing_tok, tok_row, tok_oov, eq_ids, oov_a,
                   gt_mask, gt_len, gx_off, gx_ids, masks, extra, row_counts};
        const dim3 grid((n_rows + kRowThreads / 64 - 1) / (kRowThreads / 64)), block(kRowThreads);
        hipLaunchKernelGGL(caption_ingredients_kernel, grid, block, 0, stream, a);
        const int rc = svpc_check_launch("caption_ingredients");
        if (rc) return rc;
    }
    hipLaunchKernelGGL(ingredient_totals_kernel, dim3(1), dim3(kTotThreads), 0, stream, row_counts, vid_off, n_vid, n_rows, vid_counts,
                       (u64*)acc);
    return svpc_check_launch("ingredient_totals");
}

}  // extern "C"
