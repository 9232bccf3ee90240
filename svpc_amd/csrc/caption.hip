// Evaluation tail of a decode, on the device: decoded id rows → the captions the reference submits → its repetition / diversity counts.
//
// reference: recursive_caption_dataset.py:472-500 (convert_ids_to_sentence: drop PAD / IGNORE, drop the first remaining token, keep the
// words up to the first EOS), src/translate.py:27-42 (remove_dup: runs of one word collapse), densevid_eval/evaluateRepetition.py:16-114
// (re1 … re4 per video: n-grams of every caption, none spanning two captions; a final '.' dropped, every ',' dropped),
// densevid_eval/evaluateCaptionsDiversity.py:219-282 (Div-n = distinct n-grams / unigrams), densevid_eval/get_caption_stat.py (sentence
// count, mean length, vocabulary).  The reference does this on the host with one device→host copy per sentence (translate.py:81-82).
//
// Restated by tests/caption_metrics_reference.py.  Three kernels, all integer-exact apart from the final ratios (fp64, fixed order):
//   caption_clean        one wave per id row (Lt ≤ 64, one lane per position): keep mask by ballot, compaction by prefix popcount, run
//                        collapse against the previous kept lane;
//   caption_ngram_counts one workgroup per video: the video's repetition words in LDS (≤ 4096), each gram start tests "first occurrence"
//                        against every earlier start by comparing all n ids (no hash);
//   decode_metric_accum  one workgroup: the N count rows → 8 ratios per video, summed in index order (strided partials, then a tree).
#include "common.h"

#include <climits>

namespace {

constexpr int kCleanThreads = 256;            // four rows per workgroup
constexpr int kCapWords = 4096;               // a video's S_b · Lt positions (16 KiB of words + 8 KiB of caption indices in LDS)
constexpr int kCountThreads = 256;
constexpr int kCountCols = 12;                // total_1..4, distinct_1..4, n_sen, n_words, n_empty, n_copied
constexpr int kAccCols = 13;                  // Σ re_1..4, Σ div_1..4, videos, sentences, words, empty captions, copied words

struct CleanArgs {
    const void* ids; int ids64; long long ld; int row_stride; int row_pick; int n_rows; int lt;
    long long pad, eos, ignore; int remove_dup; int* words; int* len;
};

__global__ __launch_bounds__(kCleanThreads) void caption_clean_kernel(CleanArgs a) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * (kCleanThreads / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (r >= a.n_rows) return;                    // (wave-uniform)
    const size_t src = ((size_t)r * a.row_stride + a.row_pick) * (size_t)a.ld;
    long long v64 = a.pad;
    if (lane < a.lt) v64 = a.ids64 ? ((const long long*)a.ids)[src + lane] : (long long)((const int*)a.ids)[src + lane];
    const int v = (int)v64;
    const u64 below = (1ull << lane) - 1ull;
    // 1. without PAD and IGNORE; 2. without the first of those, up to the first EOS
    u64 m = __ballot(lane < a.lt && v64 != a.pad && v64 != a.ignore);
    m &= m - 1ull;                                // (drops the lowest set bit; 0 stays 0)
    const u64 e = m & __ballot(v64 == a.eos);
    if (e) m &= (e & (0ull - e)) - 1ull;          // positions below the first EOS
    // 3. a word equal to the kept word before it belongs to that word's run
    if (a.remove_dup) {
        const u64 prev = m & below;
        const int q = prev ? 63 - __clzll((long long)prev) : lane;
        const int pv = __shfl(v, q, 64);          // (every lane takes part)
        m &= ~__ballot(prev != 0ull && pv == v);
    }
    const int n = __popcll(m);
    int* out = a.words + (size_t)r * a.lt;
    if (lane >= n && lane < a.lt) out[lane] = (int)a.pad;       // slots n … Lt − 1
    if ((m >> lane) & 1ull) out[__popcll(m & below)] = v;       // slots 0 … n − 1: the two sets of slots are disjoint
    if (lane == 0) a.len[r] = n;
}

struct CountArgs {
    const int* words; const int* len; const int* vid_off; int n_vid; int lt; int period; int comma; int vocab;
    int* counts; unsigned* vocab_bits;
};

__global__ __launch_bounds__(kCountThreads) void caption_ngram_counts_kernel(CountArgs a) {
    __shared__ int w[kCapWords];                  // the video's repetition words, captions back to back
    __shared__ unsigned short cap[kCapWords];     // the caption (row of the video) each word belongs to
    __shared__ int wave_n[kCountThreads / 64];
    __shared__ int acc[kCountCols];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int row0 = a.vid_off[b], S = a.vid_off[b + 1] - row0;
    int* out = a.counts + (size_t)b * kCountCols;
    const int P = S * a.lt;
    if (S < 0 || P > kCapWords) {                 // (the host checks this; never index LDS past its end)
        if (tid < kCountCols) out[tid] = -1;
        return;
    }
    if (tid < kCountCols) acc[tid] = 0;
    int n_words = 0, n_empty = 0, n_copied = 0;
    // pass 1: positions (row, p) in order, 256 at a time; a position is a repetition word when p < len', len' = len without a final
    // period, and the word is not a comma.  Exclusive scan of the flags: ballots inside a wave, the four wave totals through LDS.
    int base = 0;
    for (int i0 = 0; i0 < P; i0 += kCountThreads) {
        const int i = i0 + tid;
        bool keep = false;
        int word = 0, s = 0;
        if (i < P) {
            s = i / a.lt;
            const int p = i - s * a.lt;
            const int* row = a.words + (size_t)(row0 + s) * a.lt;
            const int L = min(max(a.len[row0 + s], 0), a.lt);
            if (p == 0) { n_words += L; n_empty += L == 0; }
            if (p < L) {
                word = row[p];
                if (word >= a.vocab) n_copied++;
                else if (word >= 0 && a.vocab_bits) atomicOr(a.vocab_bits + (word >> 5), 1u << (word & 31));
                const int Lr = (row[L - 1] == a.period) ? L - 1 : L;
                keep = p < Lr && word != a.comma;
            }
        }
        const u64 bal = __ballot(keep);
        __syncthreads();                          // (the previous round's wave_n has been read)
        if (lane == 0) wave_n[wv] = __popcll(bal);
        __syncthreads();
        int off = base + __popcll(bal & ((1ull << lane) - 1ull));
        for (int k = 0; k < wv; ++k) off += wave_n[k];
        if (keep) { w[off] = word; cap[off] = (unsigned short)s; }
        base += wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
    }
    __syncthreads();
    const int M = base;
    // pass 2: gram start i of size n is valid when word i + n − 1 exists in the same caption; it is a first occurrence when no earlier
    // valid start j holds the same n ids.  A thread's starts are tid, tid + 256, …: the threads of a wave read the same j (LDS broadcast).
    int tot[4] = {0, 0, 0, 0}, dist[4] = {0, 0, 0, 0};
    for (int i = tid; i < M; i += kCountThreads) {
        const int ci = cap[i];
        int ni = 1;                               // the largest valid gram size at i
        while (ni < 4 && i + ni < M && cap[i + ni] == ci) ++ni;
        const int wi0 = w[i], wi1 = ni > 1 ? w[i + 1] : 0, wi2 = ni > 2 ? w[i + 2] : 0, wi3 = ni > 3 ? w[i + 3] : 0;
        int seen = 0;                             // bit n − 1: an earlier start holds the same n-gram
        const int full = (1 << ni) - 1;
        for (int j = 0; j < i && seen != full; ++j) {
            if (w[j] != wi0) continue;
            seen |= 1;
            if (ni < 2 || j + 1 >= M || cap[j + 1] != cap[j] || w[j + 1] != wi1) continue;
            seen |= 2;
            if (ni < 3 || j + 2 >= M || cap[j + 2] != cap[j] || w[j + 2] != wi2) continue;
            seen |= 4;
            if (ni < 4 || j + 3 >= M || cap[j + 3] != cap[j] || w[j + 3] != wi3) continue;
            seen |= 8;
        }
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            if (n < ni) { tot[n]++; dist[n] += !((seen >> n) & 1); }
        }
    }
    // integer sums: the order of the atomics does not matter
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        if (tot[n]) atomicAdd(&acc[n], tot[n]);
        if (dist[n]) atomicAdd(&acc[4 + n], dist[n]);
    }
    if (n_words) atomicAdd(&acc[9], n_words);
    if (n_empty) atomicAdd(&acc[10], n_empty);
    if (n_copied) atomicAdd(&acc[11], n_copied);
    __syncthreads();
    if (tid == 8) out[8] = S;
    else if (tid < kCountCols) out[tid] = acc[tid];
}

__global__ __launch_bounds__(kCountThreads) void decode_metric_accum_kernel(const int* __restrict__ counts, int n_vid, double* __restrict__ accum) {
    __shared__ double sh[kAccCols][kCountThreads];
    const int tid = threadIdx.x;
    double v[kAccCols];
#pragma unroll
    for (int k = 0; k < kAccCols; ++k) v[k] = 0.0;
    for (int b = tid; b < n_vid; b += kCountThreads) {            // a thread's videos in index order
        const int* c = counts + (size_t)b * kCountCols;
        const double t1 = (double)c[0];
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const double t = (double)c[n], d = (double)c[4 + n];
            v[n] += c[n] > 0 ? (t - d) / t : 0.0;
            v[4 + n] += c[0] > 0 ? d / t1 : 0.0;
        }
        v[8] += 1.0;
        v[9] += (double)c[8]; v[10] += (double)c[9]; v[11] += (double)c[10]; v[12] += (double)c[11];
    }
#pragma unroll
    for (int k = 0; k < kAccCols; ++k) sh[k][tid] = v[k];
    __syncthreads();
    for (int h = kCountThreads / 2; h > 0; h >>= 1) {             // the tree: partial t takes partial t + h
        if (tid < h) {
#pragma unroll
            for (int k = 0; k < kAccCols; ++k) sh[k][tid] += sh[k][tid + h];
        }
        __syncthreads();
    }
    if (tid < kAccCols) accum[tid] += sh[tid][0];
}

}  // namespace

extern "C" {

int svpc_caption_clean(const void* ids, int ids64, long long ld, int row_stride, int row_pick, int n_rows, int lt, long long pad,
                       long long eos, long long ignore, int remove_dup, int* words, int* len, hipStream_t stream) {
    if (n_rows == 0) return 0;
    SVPC_REQUIRE(lt >= 1 && lt <= 64, "caption_clean: rows of 1..64 positions (one lane per position)");
    SVPC_REQUIRE(ld >= lt && row_stride >= 1 && row_pick >= 0 && row_pick < row_stride, "caption_clean: ld >= Lt and 0 <= row_pick < row_stride");
    SVPC_REQUIRE(n_rows > 0 && ids && words && len, "caption_clean: buffers are required");
    SVPC_REQUIRE(pad >= INT_MIN && pad <= INT_MAX, "caption_clean: pad must fit 32 bits (it fills the output rows)");
    CleanArgs a{ids, ids64, ld, row_stride, row_pick, n_rows, lt, pad, eos, ignore, remove_dup, words, len};
    const dim3 grid((n_rows + kCleanThreads / 64 - 1) / (kCleanThreads / 64)), block(kCleanThreads);
    hipLaunchKernelGGL(caption_clean_kernel, grid, block, 0, stream, a);
    return svpc_check_launch("caption_clean");
}

int svpc_caption_ngram_counts(const int* words, const int* len, const int* vid_off, int n_vid, int lt, int period, int comma, int vocab,
                              int* counts, unsigned* vocab_bits, hipStream_t stream) {
    if (n_vid == 0) return 0;
    SVPC_REQUIRE(lt >= 1 && lt <= 64 && n_vid > 0, "caption_ngram_counts: rows of 1..64 positions");
    SVPC_REQUIRE(words && len && vid_off && counts, "caption_ngram_counts: buffers are required");
    SVPC_REQUIRE(vocab >= 0, "caption_ngram_counts: vocabulary size must be >= 0");
    CountArgs a{words, len, vid_off, n_vid, lt, period, comma, vocab, counts, vocab_bits};
    hipLaunchKernelGGL(caption_ngram_counts_kernel, dim3(n_vid), dim3(kCountThreads), 0, stream, a);
    return svpc_check_launch("caption_ngram_counts");
}

int svpc_decode_metric_accum(const int* counts, int n_vid, double* acc, hipStream_t stream) {
    if (n_vid == 0) return 0;
    SVPC_REQUIRE(n_vid > 0 && counts && acc, "decode_metric_accum: buffers are required");
    hipLaunchKernelGGL(decode_metric_accum_kernel, dim3(1), dim3(kCountThreads), 0, stream, counts, n_vid, acc);
    return svpc_check_launch("decode_metric_accum");
}

}  // extern "C"
