// Consensus (minimum Bayes risk) selection among the K decoded candidates of a sentence or of a video, on the device.
//
// A group holds K ≤ 16 candidates; candidate i's utility against candidate j is the six scores of DESIGN §11.6 (Bleu_1…4, ROUGE_L, CIDEr)
// with i as the hypothesis and j as the single (pseudo-)reference; the pick is the candidate with the highest expected utility over the
// others.  Tokens, gram keys, the gram → idf table and the arithmetic are those of caption_scores.hip; a pseudo-reference's length and
// CIDEr norms are computed here by the same formulas.
//   consensus_tokens_kernel       one workgroup per stream: caption_tokens_kernel's scan over the clean rows first, first + stride, … of a
//                                 stream table (a candidate's rows are K apart in a (T, K, Lt) decode), 16-bit tokens out;
//   consensus_pair_sums_kernel    one workgroup per (group, hypothesis i) — a group's K hypotheses spread over K compute units: the K streams
//                                 in LDS (≤ 32.1 KiB); a wave per j for the LCS of i and j; a thread's ≤ 4 gram starts of i are counted in
//                                 i once (first occurrences, counts, idf — kept in registers) and then in every j, four positions per
//                                 64-bit LDS read; fp64 sums by butterfly and the four waves in order; raw sums and i's norms out;
//   consensus_pair_finish_kernel  thread per ordered pair (i, j): the six scores from the raw sums and the norms of i and of j;
//   consensus_pick_kernel         one wave per group: the candidates' weights, the expected utilities (j ascending), the arg max (ties to
//                                 the lowest index), and the gather of the chosen rows of ids / scores / lengths.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kCapTok = 1024;                 // tokens of one stream
constexpr int kStride = kCapTok + 4;          // a stream in LDS: zero-padded by 4 for the gram scan
constexpr int kMaxK = 16;
constexpr int kScoreCols = 6;                 // Bleu_1..4, ROUGE_L, CIDEr
constexpr int kCapCopied = 128;
constexpr int kVidCols = 12;                  // the plan's row per video (caption_scores.hip): X and oov0 are columns 2 and 3
constexpr int kChunk = kCapTok / 64;          // LCS columns per lane at the cap
constexpr int kNoTok = 0xFFFF;                // never a token id: a gram field past the hypothesis's end
constexpr int kSlots = kCapTok / kThreads;    // gram starts of one stream per thread

struct TokArgs {
    const int* words; const int* len; long long n_rows; const int* streams; int n_streams; int lt; int vocab;
    const int* voc_off; const int* voc_tok; int n_voc_tok; const int* vid; int n_vid; const int* oov_off; int n_oov_off; const int* oov_tok;
    int n_oov_tok; unsigned short* tokens; int* tok_len;
};

__global__ __launch_bounds__(kThreads) void consensus_tokens_kernel(TokArgs a) {
    __shared__ int wave_n[kThreads / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int* st = a.streams + (size_t)b * 4;    // first row, rows, row stride, video
    const long long row0 = st[0], stride = st[2];
    int S = max(st[1], 0);
    const int v = st[3];
    if (row0 < 0 || stride < 1 || v < 0 || v >= a.n_vid || (S > 0 && row0 + (long long)(S - 1) * stride >= a.n_rows)) S = 0;   // (never past the rows)
    const int* vd = a.vid + (size_t)max(min(v, a.n_vid - 1), 0) * kVidCols;
    const int X = min(max(vd[2], 0), kCapCopied), o0 = vd[3];
    unsigned short* out = a.tokens + (size_t)b * kCapTok;
    const int P = S * a.lt;
    int base = 0;                                 // tokens before this round's positions (uniform)
    for (int i0 = 0; i0 < P; i0 += kThreads) {
        const int i = i0 + tid;
        int cnt = 0;
        const int* src = nullptr;
        if (i < P) {
            const int s = i / a.lt, p = i - s * a.lt;
            const long long r = row0 + (long long)s * stride;
            const int L = min(max(a.len[r], 0), a.lt);
            if (p < L) {
                const int w = a.words[(size_t)r * a.lt + p];
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
            if (off + k < kCapTok) { const int t = src[k]; out[off + k] = (unsigned short)((t < 1 || t >= kNoTok) ? kNoTok : t); }
        }
        base += wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
    }
    for (int i = min(base, kCapTok) + tid; i < kCapTok; i += kThreads) out[i] = 0;
    if (tid == 0) a.tok_len[b] = base <= kCapTok ? base : -1;        // (the host refuses what could overflow)
}

struct PairArgs {
    const unsigned short* tokens; const int* tok_len; int n_grp; int K; const u64* tab_key; const double* tab_idf; int tab_cap;
    double log_docs; const double* gauss; double* out; double* work;
};

__device__ __forceinline__ u64 gram_hash(u64 key) {
    const u64 h = key * 0x9E3779B97F4A7C15ull;
    return h ^ (h >> 32);
}

// idf of a gram: one probe sequence of the host's open-addressing table (linear, key 0 = empty slot); absent: ln N
__device__ __forceinline__ double gram_idf(const PairArgs& a, u64 key) {
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

// occurrences in T[0 … m − 1] (8-byte aligned, zero-padded to a multiple of 4 and by 4 more) of the grams whose 64-bit key's low 16 n bits
// are `key`'s, n = 1 … 4 (an absent field of `key` is kNoTok, which no token is); `before`: bit n − 1 set when one starts below `self`.
// Four positions per 64-bit LDS read, no branch: position j + k's window is the four tokens from there on.
template <bool kSelf>
__device__ __forceinline__ void gram_scan(const unsigned short* T, int m, u64 key, int self, int (&c)[4], int& before) {
    const u64* T8 = reinterpret_cast<const u64*>(T);
    u64 lo = T8[0];
    for (int j = 0; j < m; j += 4) {
        const u64 hi = T8[(j >> 2) + 1];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const u64 x = (k ? (lo >> (16 * k)) | (hi << (64 - 16 * k)) : lo) ^ key;
            const int m0 = (x & 0xFFFFull) == 0ull, m1 = (x & 0xFFFFFFFFull) == 0ull, m2 = (x & 0xFFFFFFFFFFFFull) == 0ull, m3 = x == 0ull;
            c[0] += m0; c[1] += m1; c[2] += m2; c[3] += m3;
            if (kSelf && j + k < self) before |= m0 | (m1 << 1) | (m2 << 2) | (m3 << 3);
        }
        lo = hi;
    }
}

// workgroup (g, i): the sums of hypothesis i against every candidate j of group g.  out[g][i][j] takes them raw — the four CIDEr
// numerators, the four clipped counts (16 bits each) and the LCS as bit patterns — for consensus_pair_finish_kernel, which needs every
// candidate's norms; work[g][i] takes i's four squared norms.
__global__ __launch_bounds__(kThreads) void consensus_pair_sums_kernel(PairArgs a) {
    extern __shared__ __align__(16) unsigned short tok[];     // K streams of kStride tokens (a stream starts on an 8-byte boundary)
    __shared__ int sh_len[kMaxK];                 // (a stream over the cap counts as empty here; the finish writes its pairs' zeros)
    __shared__ int sh_corr[kMaxK * 4];
    __shared__ int sh_lcs[kMaxK];
    __shared__ double red[kThreads / 64][kMaxK * 4 + 4];
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int K = a.K, g = blockIdx.x / K, i = blockIdx.x - g * K;
    if (tid < K) {
        const int h = a.tok_len[(size_t)g * K + tid];
        sh_len[tid] = (h < 0 || h > kCapTok) ? 0 : h;         // (never index LDS past a stream's end)
    }
    if (tid < K * 4) sh_corr[tid] = 0;
    __syncthreads();
    for (int k = 0; k < K; ++k) {
        const int n = sh_len[k];
        const unsigned short* src = a.tokens + ((size_t)g * K + k) * kCapTok;
        for (int x = tid; x < kStride; x += kThreads) tok[k * kStride + x] = x < n ? src[x] : (unsigned short)0;
    }
    __syncthreads();
    const int H = sh_len[i];
    const unsigned short* hyp = tok + i * kStride;

    // ---- LCS of i and every other j (a wave per pair): row x of the table is the prefix maximum over y of
    //      max(L[x − 1][y], L[x − 1][y − 1] + eq(x, y)); lane l holds the columns l · chunk … l · chunk + chunk − 1 of stream j
    for (int j = wv; j < K; j += kThreads / 64) { // (wave-uniform)
        if (j == i) {
            if (lane == 63) sh_lcs[j] = H;
            continue;
        }
        const int m = sh_len[j];
        const unsigned short* ref = tok + j * kStride;
        const int chunk = __builtin_amdgcn_readfirstlane(max((m + 63) / 64, 1));
        int rt[kChunk], row[kChunk];              // row[c]: L[x − 1][y] before the maximum with `floor_`
#pragma unroll
        for (int c = 0; c < kChunk; ++c) {
            const int y = lane * chunk + c;
            rt[c] = (c < chunk && y < m) ? (int)ref[y] : 0;
            row[c] = 0;
        }
        int floor_ = 0, last = 0;                 // floor_: L[x − 1][l · chunk − 1], the prefix maximum of the lanes below
        for (int x = 0; x < H; ++x) {
            const int t = hyp[x];
            int diag = floor_, run = 0;
#pragma unroll
            for (int c = 0; c < kChunk; ++c) {
                if (c < chunk) {
                    const int up = max(row[c], floor_);
                    run = max(run, max(up, diag + (rt[c] == t ? 1 : 0)));
                    diag = up;
                    row[c] = run;
                }
            }
            int pm = run;                         // inclusive prefix maximum over the lanes
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int u = __shfl_up(pm, d, 64);
                if (lane >= d) pm = max(pm, u);
            }
            const int below = __shfl_up(pm, 1, 64);
            floor_ = lane ? below : 0;
            last = pm;
        }
        if (lane == 63) sh_lcs[j] = last;
    }

    // ---- grams: i's starts tid, tid + 256, … are counted in i once (first occurrences, counts, idf), then in every candidate j
    int ch[kSlots][4], first[kSlots];
    u64 gram[kSlots];                             // the start's four tokens as a key, kNoTok past the stream's end
    double idf[kSlots][4];
    double nh2[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < kSlots; ++q) {
        const int p = tid + q * kThreads;
        first[q] = 0;
#pragma unroll
        for (int n = 0; n < 4; ++n) { ch[q][n] = 0; idf[q][n] = 0.0; }
        gram[q] = ~0ull;
        if (p < H) {
            const int ni = min(4, H - p);
            gram[q] = 0ull;
#pragma unroll
            for (int n = 0; n < 4; ++n) gram[q] |= (u64)(n < ni ? (int)hyp[p + n] : kNoTok) << (16 * n);
            int before = 0;
            gram_scan<true>(hyp, H, gram[q], p, ch[q], before);
            first[q] = ~before & ((1 << ni) - 1);             // bit n − 1: this start is the first occurrence of its n-gram
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                if (n < ni && ((first[q] >> n) & 1)) {
                    idf[q][n] = gram_idf(a, gram[q] & (~0ull >> (48 - 16 * n)));
                    const double vh = (double)ch[q][n] * idf[q][n];
                    nh2[n] += vh * vh;
                }
            }
        }
    }
    // the fp64 sums: a butterfly over the wave's lanes, then the four wave values in order — the same inputs give the same bits
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        double v = nh2[n];
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
        if (lane == 0) red[wv][kMaxK * 4 + n] = v;
    }
    for (int j = 0; j < K; ++j) {                 // (uniform)
        const int R = sh_len[j];
        const unsigned short* ref = tok + j * kStride;
        double num[4] = {0.0, 0.0, 0.0, 0.0};
        int corr[4] = {0, 0, 0, 0};
#pragma unroll
        for (int q = 0; q < kSlots; ++q) {
            if (first[q]) {
                int cr[4] = {0, 0, 0, 0}, unused = 0;
                gram_scan<false>(ref, R, gram[q], 0, cr, unused);
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    if ((first[q] >> n) & 1) {
                        corr[n] += min(ch[q][n], cr[n]);
                        const double vh = (double)ch[q][n] * idf[q][n], vr = (double)cr[n] * idf[q][n];
                        num[n] += fmin(vh, vr) * vr;
                    }
                }
            }
        }
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            if (corr[n]) atomicAdd(&sh_corr[j * 4 + n], corr[n]);                 // integers: any order gives the same sum
            double v = num[n];
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
            if (lane == 0) red[wv][j * 4 + n] = v;
        }
    }
    __syncthreads();
    if (tid < K * 4) {                            // numerator n of the pair (i, j = tid / 4)
        a.out[((size_t)blockIdx.x * K + (tid >> 2)) * kScoreCols + (tid & 3)] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    } else if (tid >= 64 && tid < 64 + K) {
        const int j = tid - 64;                   // clipped counts ≤ 1,024 each
        const u64 packed = (u64)sh_corr[j * 4] | (u64)sh_corr[j * 4 + 1] << 16 | (u64)sh_corr[j * 4 + 2] << 32 | (u64)sh_corr[j * 4 + 3] << 48;
        double* o = a.out + ((size_t)blockIdx.x * K + j) * kScoreCols;
        o[4] = __longlong_as_double((long long)packed);
        o[5] = __longlong_as_double((long long)sh_lcs[j]);
    } else if (tid >= 128 && tid < 132) {
        const int c = kMaxK * 4 + tid - 128;
        a.work[(size_t)blockIdx.x * 4 + tid - 128] = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
    }
}

// thread (g, i, j): the six scores of the ordered pair — hypothesis i, the one reference j — from the raw sums, in place
__global__ __launch_bounds__(kThreads) void consensus_pair_finish_kernel(PairArgs a) {
    const int K = a.K;
    const long long idx = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= (long long)a.n_grp * K * K) return;
    const long long gi = idx / K;                 // g · K + i
    const int j = (int)(idx - gi * K);
    const long long gj = gi / K * K + j;
    double* out_s = a.out + (size_t)idx * kScoreCols;
    const int H = a.tok_len[gi], R = a.tok_len[gj];
    if (H < 0 || H > kCapTok || R < 0 || R > kCapTok) {       // a stream over the cap (the host refuses what could get there)
#pragma unroll
        for (int k = 0; k < kScoreCols; ++k) out_s[k] = 0.0;
        return;
    }
    double num[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) num[n] = out_s[n];
    const u64 packed = (u64)__double_as_longlong(out_s[4]);
    const int lcs = (int)__double_as_longlong(out_s[5]);
    const double tiny = 1e-15, small = 1e-9;
    const double ratio = ((double)H + tiny) / ((double)R + small);
    const double bp = ratio < 1.0 ? exp(1.0 - 1.0 / ratio) : 1.0;
    double bl = 1.0;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const int guess = max(0, H - n), corr = (int)((packed >> (16 * n)) & 0xFFFFull);
        bl *= ((double)corr + tiny) / ((double)guess + small);
        double root = n == 0 ? bl : n == 1 ? sqrt(bl) : n == 2 ? cbrt(bl) : sqrt(sqrt(bl));
        if (ratio < 1.0) root *= bp;
        out_s[n] = root;
    }
    const double beta2 = 1.2 * 1.2;
    const double p = (double)lcs / (double)max(H, 1);
    const double q = R > 0 ? (double)lcs / (double)R : 0.0;                        // an empty pseudo-reference: q = 0
    out_s[4] = (p != 0.0 && q != 0.0) ? (1.0 + beta2) * p * q / (q + beta2 * p) : 0.0;
    const int lh = max(H - 1, 0), lr = max(R - 1, 0);                              // `length`: the number of bigrams
    double total = 0.0;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const double nh = sqrt(a.work[gi * 4 + n]), nr = sqrt(a.work[gj * 4 + n]); // the pseudo-reference's norm by the same formula
        double val = num[n];
        if (nh != 0.0 && nr != 0.0) val /= nh * nr;
        total += val * a.gauss[min(abs(lh - lr), kCapTok - 1)];
    }
    out_s[5] = 10.0 * (total / 4.0);
}

struct PickArgs {
    const double* pair; int n_grp; int K; int col; int posterior; const float* scores; const int* grp_off; long long n_rows;
    const void* ids; int ids64; int lt; const long long* lengths;
    int* pick; double* expected; long long* out_ids; long long* row_pick; float* out_scores; long long* out_len;
};

__global__ __launch_bounds__(64) void consensus_pick_kernel(PickArgs a) {
    __shared__ double sh_c[kMaxK], sh_e[kMaxK];
    __shared__ int sh_pick;
    const int g = blockIdx.x, lane = threadIdx.x, K = a.K;
    long long r0 = a.grp_off[g], r1 = a.grp_off[g + 1];
    if (r0 < 0 || r1 < r0 || r1 > a.n_rows) r0 = r1 = 0;                             // (never past the rows)
    if (lane < K) {
        double c = 0.0;
        if (a.posterior) {
            for (long long r = r0; r < r1; ++r) c += (double)a.scores[r * K + lane];  // the group's sentences in order
        }
        sh_c[lane] = c;
    }
    __syncthreads();
    if (lane < K) {
        double m = sh_c[0];
        for (int j = 1; j < K; ++j) m = fmax(m, sh_c[j]);
        const bool flat = !a.posterior || m == -INFINITY;                           // every weight 1
        const double* u = a.pair + ((size_t)g * K + lane) * K * kScoreCols + a.col;
        double num = 0.0, den = 0.0;
        for (int j = 0; j < K; ++j) {
            if (j == lane) continue;
            const double w = flat ? 1.0 : exp(sh_c[j] - m);
            num += w * u[(size_t)j * kScoreCols];
            den += w;
        }
        const double e = den != 0.0 ? num / den : 0.0;
        sh_e[lane] = e;
        a.expected[(size_t)g * K + lane] = e;
    }
    __syncthreads();
    if (lane == 0) {
        int best = 0;
        for (int i = 1; i < K; ++i) {
            if (sh_e[i] > sh_e[best]) best = i;                                     // ties go to the lowest index
        }
        sh_pick = best;
        a.pick[g] = best;
    }
    __syncthreads();
    const int k = sh_pick;
    if (!a.out_ids) return;
    for (long long r = r0; r < r1; ++r) {         // the chosen row of every sentence of the group
        const size_t src = ((size_t)r * K + k) * a.lt;
        if (lane < a.lt) {
            a.out_ids[(size_t)r * a.lt + lane] = a.ids64 ? ((const long long*)a.ids)[src + lane] : (long long)((const int*)a.ids)[src + lane];
        }
        if (lane == 0) {
            a.row_pick[r] = k;
            if (a.out_scores) a.out_scores[r] = a.scores[r * K + k];
            if (a.out_len) a.out_len[r] = a.lengths[r * K + k];
        }
    }
}

}  // namespace

extern "C" {

int svpc_consensus_tokens(const int* words, const int* len, long long n_rows, const int* streams, int n_streams, int lt, int vocab,
                          const int* voc_off, const int* voc_tok, int n_voc_tok, const int* vid, int n_vid, const int* oov_off, int n_oov_off,
                          const int* oov_tok, int n_oov_tok, unsigned short* tokens, int* tok_len, hipStream_t stream) {
    if (n_streams == 0) return 0;
    SVPC_REQUIRE(lt >= 1 && lt <= 64 && n_streams > 0 && vocab >= 1 && n_vid >= 1 && n_rows >= 0, "consensus_tokens: rows of 1..64 positions, a vocabulary, videos");
    SVPC_REQUIRE(n_voc_tok >= 0 && n_oov_off >= 0 && n_oov_tok >= 0, "consensus_tokens: table sizes out of range");
    SVPC_REQUIRE(words && len && streams && voc_off && voc_tok && vid && oov_off && oov_tok && tokens && tok_len,
                 "consensus_tokens: buffers are required");
    TokArgs a{words, len, n_rows, streams, n_streams, lt, vocab, voc_off, voc_tok, n_voc_tok, vid, n_vid, oov_off, n_oov_off, oov_tok, n_oov_tok,
              tokens, tok_len};
    hipLaunchKernelGGL(consensus_tokens_kernel, dim3(n_streams), dim3(kThreads), 0, stream, a);
    return svpc_check_launch("consensus_tokens");
}

int svpc_consensus_pair_scores(const unsigned short* tokens, const int* tok_len, int n_grp, int k, const unsigned long long* tab_key,
                               const double* tab_idf, int tab_cap, double log_docs, const double* gauss, double* out, double* work,
                               hipStream_t stream) {
    if (n_grp == 0) return 0;
    SVPC_REQUIRE(n_grp > 0 && k >= 1 && k <= kMaxK, "consensus_pair_scores: groups of 1..16 candidates");
    SVPC_REQUIRE(tab_cap >= 2 && (tab_cap & (tab_cap - 1)) == 0, "consensus_pair_scores: the gram table's capacity is a power of two");
    SVPC_REQUIRE(n_grp <= 0x7fffffff / (k * k), "consensus_pair_scores: too many groups");
    SVPC_REQUIRE(tokens && tok_len && tab_key && tab_idf && gauss && out && work, "consensus_pair_scores: buffers are required");
    PairArgs a{tokens, tok_len, n_grp, k, (const u64*)tab_key, tab_idf, tab_cap, log_docs, gauss, out, work};
    hipLaunchKernelGGL(consensus_pair_sums_kernel, dim3(n_grp * k), dim3(kThreads), (size_t)k * kStride * sizeof(unsigned short), stream, a);
    const int rc = svpc_check_launch("consensus_pair_scores");
    if (rc) return rc;
    hipLaunchKernelGGL(consensus_pair_finish_kernel, dim3((n_grp * k * k + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, a);
    return svpc_check_launch("consensus_pair_scores");
}

int svpc_consensus_pick(const double* pair, int n_grp, int k, int col, int posterior, const float* scores, const int* grp_off,
                        long long n_rows, const void* ids, int ids64, int lt, const long long* lengths, int* pick, double* expected,
                        long long* out_ids, long long* row_pick, float* out_scores, long long* out_len, hipStream_t stream) {
    if (n_grp == 0) return 0;
    SVPC_REQUIRE(n_grp > 0 && k >= 1 && k <= kMaxK && col >= 0 && col < kScoreCols && n_rows >= 0, "consensus_pick: groups of 1..16 candidates, a utility column 0..5");
    SVPC_REQUIRE(pair && grp_off && pick && expected, "consensus_pick: buffers are required");
    SVPC_REQUIRE(!posterior || scores, "consensus_pick: posterior weights need the candidates' scores");
    SVPC_REQUIRE(!out_ids || (ids && row_pick && lt >= 1 && lt <= 64), "consensus_pick: the gather needs ids of 1..64 positions and row_pick");
    SVPC_REQUIRE((!out_scores || (scores && out_ids)) && (!out_len || (lengths && out_ids)), "consensus_pick: gathered scores / lengths need their sources");
    PickArgs a{pair, n_grp, k, col, posterior, scores, grp_off, n_rows, ids, ids64, lt, lengths, pick, expected, out_ids, row_pick, out_scores, out_len};
    hipLaunchKernelGGL(consensus_pick_kernel, dim3(n_grp), dim3(64), 0, stream, a);
    return svpc_check_launch("consensus_pick");
}

}  // extern "C"
