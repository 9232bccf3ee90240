// Bleu_1…4, ROUGE_L and CIDEr of decoded captions against reference paragraphs, on the device.
//
// reference: src/train.py:278-331 (eval_language_metrics: decode, write JSON, run densevid_eval/para-evaluate.py in a subprocess),
// :409-455 (the early stop on CIDEr); densevid_eval/para-evaluate.py:26-29 (parse_sent), :71-84 (a video's hypothesis paragraph),
// :112-125 (evaluate_para).  The scorers are the published arithmetic as the public caption scorer implements it — Bleu(4) with option
// `closest`, Rouge with β = 1.2, Cider() with n = 4 and σ = 6 — stated in DESIGN §11.6 and restated by tests/caption_scores_reference.py.
//
// A token is an id 1 … 65534 of the host's token lexicon (svpc_amd/caption_scores.py); an n-gram is the 64-bit key of its ≤ 4 ids in 16-bit
// fields (first token lowest, absent fields 0), so grams are compared exactly.  The gram → idf table is built on the host and only probed
// here; the hash is stated in include/svpc_hip.h (gram_hash below).
//   caption_tokens_kernel        one workgroup per video: every clean word's token count (vocabulary CSR below V, the video's CSR from V
//                                on), a scan over the S_b · Lt positions (shuffles inside a wave, the four wave totals through LDS), scatter;
//   caption_score_counts_kernel  one workgroup per video: hypothesis and ≤ 4 references in LDS (10 KiB); a thread's gram starts count
//                                their grams (n = 1 … 4 at once) in the hypothesis and in every reference and probe the idf once per
//                                gram; first occurrences give the clipped counts (integers) and the CIDEr sums (fp64, fixed order);
//                                wave r runs the LCS against reference r; thread 0 finishes the six scores;
//   caption_score_accum_kernel   one workgroup: 64-bit integer totals, Σ ROUGE_L and Σ CIDEr in index order per thread, then a fixed tree.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kCapTok = 1024;                 // tokens of a hypothesis and of a reference
constexpr int kMaxRefs = 4;
constexpr int kVidCols = 12;                  // n_ref, corpus index, X, oov0, ref_off[4], ref_len[4]
constexpr int kCountCols = 11;                // correct_1..4, guess_1..4, testlen, reflen, lcs
constexpr int kScoreCols = 6;                 // Bleu_1..4, ROUGE_L, CIDEr
constexpr int kCapCopied = 128;
constexpr int kChunk = kCapTok / 64;          // LCS columns per lane at the cap
constexpr int kNoTok = 0xFFFF;                // never a token id: a gram field past the hypothesis's end
constexpr int kSums = 4 + 4 * kMaxRefs;       // norm_h,n² and the CIDEr numerators per (reference, n)

struct TokArgs {
    const int* words; const int* len; const int* vid_off; int n_vid; int lt; int vocab;
    const int* voc_off; const int* voc_tok; int n_voc_tok; const int* vid; const int* oov_off; int n_oov_off; const int* oov_tok; int n_oov_tok;
    int* tokens; int* tok_len;
};

__global__ __launch_bounds__(kThreads) void caption_tokens_kernel(TokArgs a) {
    __shared__ int wave_n[kThreads / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int row0 = a.vid_off[b], S = max(a.vid_off[b + 1] - row0, 0);
    const int* vd = a.vid + (size_t)b * kVidCols;
    const int X = min(max(vd[2], 0), kCapCopied), o0 = vd[3];
    int* out = a.tokens + (size_t)b * kCapTok;
    const int P = S * a.lt;
    int base = 0;                                 // tokens before this round's positions (uniform)
    for (int i0 = 0; i0 < P; i0 += kThreads) {
        const int i = i0 + tid;
        int cnt = 0;
        const int* src = nullptr;
        if (i < P) {
            const int s = i / a.lt, p = i - s * a.lt;
            const int L = min(max(a.len[row0 + s], 0), a.lt);
            if (p < L) {
                const int w = a.words[(size_t)(row0 + s) * a.lt + p];
                int t0 = 0, t1 = 0, cap = 0;
                const int* tok = nullptr;
                if (w >= 0 && w < a.vocab) { t0 = a.voc_off[w]; t1 = a.voc_off[w + 1]; cap = a.n_voc_tok; tok = a.voc_tok; }
                else {
                    const int x = w - a.vocab;    // a copied word of this video; any other id spells nothing
                    if (x >= 0 && x < X && o0 >= 0 && o0 + x + 1 < a.n_oov_off) {
                        t0 = a.oov_off[o0 + x]; t1 = a.oov_off[o0 + x + 1]; cap = a.n_oov_tok; tok = a.oov_tok;
                    }
                }
                if (tok && t0 >= 0 && t1 > t0 && t1 <= cap) { cnt = t1 - t0; src = tok + t0; }
            }
        }
        int inc = cnt;                            // inclusive scan inside the wave (every lane takes part)
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(inc, d, 64);
            if (lane >= d) inc += t;
        }
        __syncthreads();                          // (the previous round's wave_n has been read)
        if (lane == 63) wave_n[wv] = inc;
        __syncthreads();
        int off = base + inc - cnt;
        for (int k = 0; k < wv; ++k) off += wave_n[k];
        for (int k = 0; k < cnt; ++k) {
            if (off + k < kCapTok) out[off + k] = src[k];
        }
        base += wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
    }
    for (int i = min(base, kCapTok) + tid; i < kCapTok; i += kThreads) out[i] = 0;
    if (tid == 0) a.tok_len[b] = base <= kCapTok ? base : -1;        // (the host refuses what could overflow)
}

struct ScoreArgs {
    const int* tokens; const int* tok_len; int n_vid; const int* vid; const double* ref_norm; const unsigned short* ref_tok;
    long long n_ref_tok; const u64* tab_key; const double* tab_idf; int tab_cap; double log_docs; const double* gauss;
    int* counts; double* scores; long long* seen; int n_seen;
};

__device__ __forceinline__ u64 gram_hash(u64 key) {
    const u64 h = key * 0x9E3779B97F4A7C15ull;
    return h ^ (h >> 32);
}

// idf of a gram: one probe sequence of the host's open-addressing table (linear, key 0 = empty slot); absent: ln N
__device__ __forceinline__ double gram_idf(const ScoreArgs& a, u64 key) {
    const u64 mask = (u64)a.tab_cap - 1ull;
    u64 slot = gram_hash(key) & mask;
    for (int p = 0; p < a.tab_cap; ++p) {
        const u64 k = a.tab_key[slot];
        if (k == key) return a.tab_idf[slot];
        if (k == 0ull) break;
        slot = (slot + 1ull) & mask;
    }
    return a.log_docs;
}

// occurrences in T[0 … m − 1] (zero-padded by 4) of the grams (t0), (t0 t1), … ; `before`: bit n − 1 set when one starts below `self`
__device__ __forceinline__ void gram_scan(const unsigned short* T, int m, int t0, int t1, int t2, int t3, int self, int (&c)[4], int& before) {
    for (int j = 0; j < m; ++j) {
        if (T[j] != t0) continue;
        c[0]++; before |= j < self ? 1 : 0;
        if (T[j + 1] != t1) continue;
        c[1]++; before |= j < self ? 2 : 0;
        if (T[j + 2] != t2) continue;
        c[2]++; before |= j < self ? 4 : 0;
        if (T[j + 3] != t3) continue;
        c[3]++; before |= j < self ? 8 : 0;
    }
}

__global__ __launch_bounds__(kThreads) void caption_score_counts_kernel(ScoreArgs a) {
    __shared__ unsigned short hyp[kCapTok + 4];
    __shared__ unsigned short ref[kMaxRefs][kCapTok + 4];
    __shared__ int sh_corr[4];
    __shared__ int sh_lcs[kMaxRefs];
    __shared__ double red[kThreads / 64][kSums];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int* vd = a.vid + (size_t)b * kVidCols;
    int* out_c = a.counts + (size_t)b * kCountCols;
    double* out_s = a.scores + (size_t)b * kScoreCols;
    const int H = a.tok_len[b];
    const int n_ref = min(max(vd[0], 0), kMaxRefs);
    if (H < 0 || H > kCapTok) {                   // (a hypothesis over the cap: the host refuses it; never index LDS past its end)
        if (tid < kCountCols) out_c[tid] = -1;
        if (tid < kScoreCols) out_s[tid] = 0.0;
        return;
    }
    int rlen[kMaxRefs];
    long long roff[kMaxRefs];
#pragma unroll
    for (int r = 0; r < kMaxRefs; ++r) {
        roff[r] = vd[4 + r];
        rlen[r] = r < n_ref ? vd[8 + r] : 0;
        if (rlen[r] < 0 || rlen[r] > kCapTok || roff[r] < 0 || roff[r] + rlen[r] > a.n_ref_tok) rlen[r] = 0;
    }
    for (int i = tid; i < kCapTok + 4; i += kThreads) {
        int t = 0;
        if (i < H) { t = a.tokens[(size_t)b * kCapTok + i]; if (t < 1 || t >= kNoTok) t = kNoTok; }
        hyp[i] = (unsigned short)t;
#pragma unroll
        for (int r = 0; r < kMaxRefs; ++r) ref[r][i] = i < rlen[r] ? a.ref_tok[roff[r] + i] : (unsigned short)0;
    }
    if (tid < 4) sh_corr[tid] = 0;
    if (tid < kMaxRefs) sh_lcs[tid] = 0;
    __syncthreads();

    // ---- grams: a thread's starts tid, tid + 256, … in index order
    int corr[4] = {0, 0, 0, 0};
    double nh2[4] = {0.0, 0.0, 0.0, 0.0};
    double num[kMaxRefs][4];
#pragma unroll
    for (int r = 0; r < kMaxRefs; ++r) {
#pragma unroll
        for (int n = 0; n < 4; ++n) num[r][n] = 0.0;
    }
    for (int i = tid; i < H; i += kThreads) {
        const int ni = min(4, H - i);
        const int t0 = hyp[i], t1 = ni > 1 ? hyp[i + 1] : kNoTok, t2 = ni > 2 ? hyp[i + 2] : kNoTok, t3 = ni > 3 ? hyp[i + 3] : kNoTok;
        int ch[4] = {0, 0, 0, 0}, before = 0;
        gram_scan(hyp, H, t0, t1, t2, t3, i, ch, before);
        const int first = ~before & ((1 << ni) - 1);          // bit n − 1: this start is the first occurrence of its n-gram
        if (!first) continue;
        double idf[4], vh[4];
        u64 key = 0ull;
        const int tk[4] = {t0, t1, t2, t3};
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            idf[n] = 0.0; vh[n] = 0.0;
            if (n < ni) {
                key |= (u64)tk[n] << (16 * n);
                if ((first >> n) & 1) { idf[n] = gram_idf(a, key); vh[n] = (double)ch[n] * idf[n]; }
            }
        }
        int mx[4] = {0, 0, 0, 0};
#pragma unroll
        for (int r = 0; r < kMaxRefs; ++r) {
            if (r < n_ref) {                      // (uniform)
                int cr[4] = {0, 0, 0, 0}, unused = 0;
                gram_scan(ref[r], rlen[r], t0, t1, t2, t3, 0, cr, unused);
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    if ((first >> n) & 1) {
                        mx[n] = max(mx[n], cr[n]);
                        const double vr = (double)cr[n] * idf[n];
                        num[r][n] += fmin(vh[n], vr) * vr;
                    }
                }
            }
        }
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            if ((first >> n) & 1) { corr[n] += min(ch[n], mx[n]); nh2[n] += vh[n] * vh[n]; }
        }
    }
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        if (corr[n]) atomicAdd(&sh_corr[n], corr[n]);         // integers: any order gives the same sum
    }
    // the fp64 sums: a butterfly over the wave's lanes, then the four wave values in order — the same inputs give the same bits
    double v[kSums];
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        v[n] = nh2[n];
#pragma unroll
        for (int r = 0; r < kMaxRefs; ++r) v[4 + 4 * r + n] = num[r][n];
    }
#pragma unroll
    for (int k = 0; k < kSums; ++k) {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) v[k] += __shfl_xor(v[k], d, 64);
        if (lane == 0) red[wv][k] = v[k];
    }

    // ---- LCS of the hypothesis and reference wv: row i of the table is the prefix maximum over j of
    //      max(L[i − 1][j], L[i − 1][j − 1] + eq(i, j)); lane l holds the columns l · chunk … l · chunk + chunk − 1
    if (wv < n_ref) {                             // (wave-uniform)
        const int m = wv == 0 ? rlen[0] : wv == 1 ? rlen[1] : wv == 2 ? rlen[2] : rlen[3];
        const int chunk = __builtin_amdgcn_readfirstlane(max((m + 63) / 64, 1));
        int rt[kChunk], row[kChunk];              // row[c]: L[i − 1][j] before the maximum with `floor`
#pragma unroll
        for (int c = 0; c < kChunk; ++c) {
            const int j = lane * chunk + c;
            rt[c] = (c < chunk && j < m) ? (int)ref[wv][j] : 0;
            row[c] = 0;
        }
        int floor_ = 0, last = 0;                 // floor_: L[i − 1][l · chunk − 1], the prefix maximum of the lanes below
        for (int i = 0; i < H; ++i) {
            const int x = hyp[i];
            int diag = floor_, run = 0;
#pragma unroll
            for (int c = 0; c < kChunk; ++c) {
                if (c < chunk) {
                    const int up = max(row[c], floor_);
                    run = max(run, max(up, diag + (rt[c] == x ? 1 : 0)));
                    diag = up;
                    row[c] = run;
                }
            }
            int pm = run;                         // inclusive prefix maximum over the lanes
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int t = __shfl_up(pm, d, 64);
                if (lane >= d) pm = max(pm, t);
            }
            const int below = __shfl_up(pm, 1, 64);
            floor_ = lane ? below : 0;
            last = pm;
        }
        if (lane == 63) sh_lcs[wv] = last;
    }
    __syncthreads();
    if (tid != 0) return;

    // ---- the video's counts and scores
    double s[kSums];
#pragma unroll
    for (int k = 0; k < kSums; ++k) s[k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
    int reflen = 0, best_d = 0x7fffffff, lmax = 0;
    double q = 0.0;
#pragma unroll
    for (int r = 0; r < kMaxRefs; ++r) {
        if (r < n_ref) {
            const int d = abs(rlen[r] - H);
            if (d < best_d || (d == best_d && rlen[r] < reflen)) { best_d = d; reflen = rlen[r]; }
            lmax = max(lmax, sh_lcs[r]);
            if (rlen[r] > 0) q = fmax(q, (double)sh_lcs[r] / (double)rlen[r]);
        }
    }
    const double tiny = 1e-15, small = 1e-9;
    const double ratio = ((double)H + tiny) / ((double)reflen + small);
    const double bp = ratio < 1.0 ? exp(1.0 - 1.0 / ratio) : 1.0;
    double bl = 1.0;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const int guess = max(0, H - n);
        out_c[n] = sh_corr[n];
        out_c[4 + n] = guess;
        bl *= ((double)sh_corr[n] + tiny) / ((double)guess + small);
        double root = n == 0 ? bl : n == 1 ? sqrt(bl) : n == 2 ? cbrt(bl) : sqrt(sqrt(bl));
        if (ratio < 1.0) root *= bp;
        out_s[n] = n_ref ? root : 0.0;
    }
    out_c[8] = H; out_c[9] = reflen; out_c[10] = lmax;
    const double beta2 = 1.2 * 1.2;
    const double p = (double)lmax / (double)max(H, 1);
    out_s[4] = (p != 0.0 && q != 0.0) ? (1.0 + beta2) * p * q / (q + beta2 * p) : 0.0;
    const int lh = max(H - 1, 0);                 // `length`: the number of bigrams
    double total = 0.0;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const double nh = sqrt(s[n]);
        double sn = 0.0;
#pragma unroll
        for (int r = 0; r < kMaxRefs; ++r) {
            if (r < n_ref) {
                double val = s[4 + 4 * r + n];
                const double nr = a.ref_norm[((size_t)b * kMaxRefs + r) * 4 + n];
                if (nh != 0.0 && nr != 0.0) val /= nh * nr;
                sn += val * a.gauss[min(abs(lh - max(rlen[r] - 1, 0)), kCapTok - 1)];
            }
        }
        total += sn;
    }
    out_s[5] = n_ref ? 10.0 * (total / 4.0) / (double)n_ref : 0.0;
    const int idx = vd[1];
    if (a.seen && idx >= 0 && idx < a.n_seen) a.seen[idx] = 1;
}

__global__ __launch_bounds__(kThreads) void caption_score_accum_kernel(const int* __restrict__ counts, const double* __restrict__ scores,
                                                                       int n_vid, u64* acc_i, double* acc_f) {
    __shared__ u64 tot[kCountCols];
    __shared__ double sh[2][kThreads];
    const int tid = threadIdx.x;
    if (tid < kCountCols) tot[tid] = 0ull;
    __syncthreads();
    u64 c[kCountCols];
#pragma unroll
    for (int k = 0; k < kCountCols; ++k) c[k] = 0ull;
    double rouge = 0.0, cider = 0.0;
    for (int b = tid; b < n_vid; b += kThreads) {                // a thread's videos in index order
        const int* row = counts + (size_t)b * kCountCols;
        if (row[8] < 0) continue;                 // (a refused hypothesis: counted nowhere)
#pragma unroll
        for (int k = 0; k < 10; ++k) c[k] += (u64)row[k];
        c[10] += 1ull;                            // videos
        rouge += scores[(size_t)b * kScoreCols + 4];
        cider += scores[(size_t)b * kScoreCols + 5];
    }
#pragma unroll
    for (int k = 0; k < kCountCols; ++k) {
        if (c[k]) atomicAdd(&tot[k], c[k]);
    }
    sh[0][tid] = rouge; sh[1][tid] = cider;
    __syncthreads();
    for (int h = kThreads / 2; h > 0; h >>= 1) {                 // the tree: partial t takes partial t + h
        if (tid < h) { sh[0][tid] += sh[0][tid + h]; sh[1][tid] += sh[1][tid + h]; }
        __syncthreads();
    }
    if (tid < kCountCols) acc_i[tid] += tot[tid];
    if (tid < 2) acc_f[tid] += sh[tid][0];
}

}  // namespace

extern "C" {

int svpc_caption_tokens(const int* words, const int* len, const int* vid_off, int n_vid, int lt, int vocab, const int* voc_off,
                        const int* voc_tok, int n_voc_tok, const int* vid, const int* oov_off, int n_oov_off, const int* oov_tok,
                        int n_oov_tok, int* tokens, int* tok_len, hipStream_t stream) {
    if (n_vid == 0) return 0;
    SVPC_REQUIRE(lt >= 1 && lt <= 64 && n_vid > 0 && vocab >= 1, "caption_tokens: rows of 1..64 positions, a vocabulary");
    SVPC_REQUIRE(n_voc_tok >= 0 && n_oov_off >= 0 && n_oov_tok >= 0, "caption_tokens: table sizes out of range");
    SVPC_REQUIRE(words && len && vid_off && voc_off && voc_tok && vid && oov_off && oov_tok && tokens && tok_len,
                 "caption_tokens: buffers are required");
    TokArgs a{words, len, vid_off, n_vid, lt, vocab, voc_off, voc_tok, n_voc_tok, vid, oov_off, n_oov_off, oov_tok, n_oov_tok, tokens, tok_len};
    hipLaunchKernelGGL(caption_tokens_kernel, dim3(n_vid), dim3(kThreads), 0, stream, a);
    return svpc_check_launch("caption_tokens");
}

int svpc_caption_score_counts(const int* tokens, const int* tok_len, int n_vid, const int* vid, const double* ref_norm,
                              const unsigned short* ref_tok, long long n_ref_tok, const unsigned long long* tab_key, const double* tab_idf,
                              int tab_cap, double log_docs, const double* gauss, int* counts, double* scores, long long* seen, int n_seen,
                              hipStream_t stream) {
    if (n_vid == 0) return 0;
    SVPC_REQUIRE(n_vid > 0 && n_ref_tok >= 0 && n_seen >= 0, "caption_score_counts: sizes out of range");
    SVPC_REQUIRE(tab_cap >= 2 && (tab_cap & (tab_cap - 1)) == 0, "caption_score_counts: the gram table's capacity is a power of two");
    SVPC_REQUIRE(tokens && tok_len && vid && ref_norm && ref_tok && tab_key && tab_idf && gauss && counts && scores,
                 "caption_score_counts: buffers are required");
    ScoreArgs a{tokens, tok_len, n_vid, vid, ref_norm, ref_tok, n_ref_tok, (const u64*)tab_key, tab_idf, tab_cap, log_docs, gauss,
                counts, scores, seen, n_seen};
    hipLaunchKernelGGL(caption_score_counts_kernel, dim3(n_vid), dim3(kThreads), 0, stream, a);
    return svpc_check_launch("caption_score_counts");
}

int svpc_caption_score_accum(const int* counts, const double* scores, int n_vid, unsigned long long* acc_i, double* acc_f,
                             hipStream_t stream) {
    if (n_vid == 0) return 0;
    SVPC_REQUIRE(n_vid > 0 && counts && scores && acc_i && acc_f, "caption_score_accum: buffers are required");
    hipLaunchKernelGGL(caption_score_accum_kernel, dim3(1), dim3(kThreads), 0, stream, counts, scores, n_vid, (u64*)acc_i, acc_f);
    return svpc_check_launch("caption_score_accum");
}

}  // extern "C"
