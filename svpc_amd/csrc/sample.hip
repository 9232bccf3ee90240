// Random-sampling caption decoding (the random-sampling half of the reference's OpenNMT decode-strategy lineage: random_sampling_temp,
// random_sampling_topk, random_sampling_topp; the reference vendored only BeamSearch).  One step over the T·R sample rows r = t·R + j of
// every sentence t: the decoder side is the beam decode's (svpc_attn_q1_ln_idx_fwd with a static ancestry table r·Lt + j, q_group = R),
// and every row draws its own token.  Rows are independent: one wave per row, no workgroup-wide state.
//
// One step for a live row r at position p = pos + 1 (restated by tests/sampling_reference.py::sample_select):
//   s_c   step score of column c (beam's: log p, or logit − log-sum-exp of the row without UNK; fp64, rounded once to fp32);
//   K0    columns c < C_r, c ≠ UNK, s_c > −inf, and not EOS while p ≤ min_len; order c ≻ d: higher raw value, then lower column;
//   K1    the first min(k, |K0|) columns of K0 in ≻ order (k = 0: all of K0);
//   z_c   = (double)s_c / τ;
//   K2    0 < q < 1: the shortest ≻-prefix of K1 whose Σ w ≥ q·W, w_c = exp(z_c − z_first), W = Σ_K1 w; otherwise K1;
//   pick  c* = argmax over K2 of z_c − log(−log u_c), u_c = (svpc_hash32(seed, pos, r·4096 + c) + 0.5)·2⁻³² (Gumbel-max: an exact draw
//         from softmax(z) over K2), ties to the lower column;
//   then  ext c*, model side UNK for a copied word (c* ≥ C_r − X_r), cum = fp32(cum + s_c*), len = p, finished once c* = EOS.
// A finished row takes PAD (both id spaces, step score 0, length kept); a live row with an empty K0 takes PAD, cum −inf, finished, len p.
//
// The ≻ order is the descending order of a 44-bit key (order-preserving bits of raw) << 12 | (4095 − c): distinct per column, so the k-th
// column (top-k) and the top-p cut are found by one bisection each over the key bits, MSB first — a count by ballots for top-k, an fp64
// wave sum of w for top-p (a sum of non-negative terms is monotone in each of them, so the bisection is well defined).  Columns live in
// registers, NPL per lane (column c = lane + 64·j).
//
// Truncation (svpc_sample_step_trunc; the TRUNC instantiations; restated by tests/truncation_reference.py::truncate): four further stages
// between K2 and the pick, in this order, each off at 0.  Each sees the distribution renormalised over the survivors S of the stage
// before it: first = the ≻-first column of S (it has the largest s: z is monotone in the raw value), w_c = exp(z_c − z_first), W = Σ_S w,
// q_c = w_c / W, ln q_c = (z_c − z_first) − ln W; a column with w_c = 0 adds 0 to an entropy and has ln q_c = −inf.
//   min-p    0 < a < 1: keep w_c ≥ a (w_first = 1: the first column stays);
//   typical  0 < m < 1: H = −Σ q ln q, d_c = |−ln q_c − H|, d* the smallest d with Σ_{d_c ≤ d*} q_c ≥ m (the largest d when rounding keeps
//            the whole sum below m); keep d_c ≤ d*: equal d stay or go together, the mode may go, the set is never empty;
//   epsilon  0 < ε < 1: keep q_c ≥ ε, and the first column when none does (q_first is the largest q);
//   eta      0 < η < 1: H over the current set, thr = min(η, √η·exp(−H)); keep q_c ≥ thr, and the first column when none does.
// The pick is the same Gumbel-max over what is left, and cum still adds the untruncated s.  The survivors are a bit per column and lane
// (the 44-bit keys are dead after top-p).  d ≥ 0, so its fp64 bit pattern is order-preserving: d* is one bisection over its 63 value
// bits, MSB first, an fp64 wave sum of q per probe over the d bits held in registers next to q.
#include "common.h"

#include <climits>

namespace {

constexpr int kSampleColsMax = 4096;          // the column stride of the draw index r·4096 + c; a row holds at most this many columns
constexpr int kSampleThreads = 256;           // four rows per workgroup
constexpr int kKeyBits = 44;

struct SampleArgs {
    const float* scores; int ld; const int* row_c; const int* row_x; int n_rows;
    int pos; int logits; int unk; int eos; int pad;
    double temp; int topk; double topp; int min_len; const long long* seed;
    float* cum; int* finished; int* len;
    int* text_out; int* ext_out; int ld_tok; int* next_ext; int* next_model;
    double min_p, typical_p, epsilon, eta; int* kept_out;       // (read by the TRUNC instantiations only)
};

// order-preserving unsigned image of a float (larger float ↔ larger key; NaN never reaches it: a NaN is not a candidate)
__device__ __forceinline__ unsigned ord_key(float v) {
    const unsigned b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// fp64 sum over the 64 lanes, the result in every lane: the DPP steps of wave_sum (common.h) on both halves, then the four row sums.
// All 64 lanes active (wave-uniform control flow); a fixed order, so the result is deterministic.
template <int CTRL>
__device__ __forceinline__ double dpp_add_d(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, true);
    return v + __hiloint2double(hi, lo);
}
__device__ __forceinline__ double readlane_d(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
__device__ __forceinline__ double wave_sum_dd(double v) {
    v = dpp_add_d<0xB1>(v);
    v = dpp_add_d<0x4E>(v);
    v = dpp_add_d<0x141>(v);
    v = dpp_add_d<0x140>(v);
    return (readlane_d(v, 0) + readlane_d(v, 16)) + (readlane_d(v, 32) + readlane_d(v, 48));
}
__device__ __forceinline__ double wave_max_d(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ bool has_bit(u64 set, int j) { return (set >> j) & 1ull; }

// the distribution renormalised over the columns of `alive` (bit j: column lane + 64·j): w_c = exp(z_c − z_first), 0 off the set
// → W = Σ w in wave_sum_dd's fixed order; zf = z_first
template <int NPL>
__device__ __forceinline__ double renorm(const float (&s)[NPL], u64 alive, double temp, double (&w)[NPL], double& zf) {
    float sf = -INFINITY;
#pragma unroll
    for (int j = 0; j < NPL; ++j)
        if (has_bit(alive, j)) sf = fmaxf(sf, s[j]);
    zf = (double)wave_max(sf) / temp;
    double wl = 0.0;
#pragma unroll
    for (int j = 0; j < NPL; ++j) {
        w[j] = has_bit(alive, j) ? exp((double)s[j] / temp - zf) : 0.0;
        wl += w[j];
    }
    return wave_sum_dd(wl);
}

// H = −Σ q ln q over the set, q = w / W, ln q = (z − z_first) − ln W; a column with w = 0 adds nothing
template <int NPL>
__device__ __forceinline__ double entropy(const float (&s)[NPL], const double (&w)[NPL], double temp, double zf, double W, double lnW) {
    double hl = 0.0;
#pragma unroll
    for (int j = 0; j < NPL; ++j)
        if (w[j] > 0.0) hl += (w[j] / W) * (((double)s[j] / temp - zf) - lnW);
    return -wave_sum_dd(hl);
}

// the ≻-first column of `alive` alone.  The raw values left the registers once the keys were built, so they are read again (a column
// of the set lies inside the row).
template <int NPL>
__device__ __forceinline__ u64 first_only(const float* row, int lane, u64 alive) {
    u64 best = 0; int bj = 0;
#pragma unroll
    for (int j = 0; j < NPL; ++j)
        if (has_bit(alive, j)) {
            const int c = lane + 64 * j;
            const u64 k = ((u64)ord_key(row[c]) << 12) | (u64)(kSampleColsMax - 1 - c);
            if (k > best) { best = k; bj = j; }
        }
    u64 top = best;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const u64 ot = __shfl_xor(top, o, 64);
        top = ot > top ? ot : top;
    }
    return (best != 0 && best == top) ? 1ull << bj : 0ull;       // (keys are distinct per column)
}

// keep the columns of `alive` with q = w / W ≥ thr, and the ≻-first column when none has (it holds the largest q)
template <int NPL>
__device__ __forceinline__ u64 keep_at_least(const float* row, int lane, u64 alive, const double (&w)[NPL], double W, double thr) {
    u64 keep = 0;
#pragma unroll
    for (int j = 0; j < NPL; ++j)
        if (has_bit(alive, j) && w[j] / W >= thr) keep |= 1ull << j;
    if (__ballot(keep != 0) != 0) return keep;    // (wave-uniform)
    return first_only<NPL>(row, lane, alive);
}

template <int NPL, bool TRUNC>
__global__ __launch_bounds__(kSampleThreads) void sample_step_kernel(SampleArgs a) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * (kSampleThreads / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (r >= a.n_rows) return;                    // (wave-uniform)
    const int p = a.pos + 1;
    if (a.finished[r]) {                          // (wave-uniform) a finished row carries PAD, its cum and its length forward
        if (lane == 0) {
            a.next_ext[r] = a.pad; a.next_model[r] = a.pad;
            a.text_out[(size_t)r * a.ld_tok + p] = a.pad; a.ext_out[(size_t)r * a.ld_tok + p] = a.pad;
            if constexpr (TRUNC)
                if (a.kept_out) a.kept_out[r] = 0;
        }
        return;
    }
    const int C = a.row_c[r], X = a.row_x[r];
    const float* row = a.scores + (size_t)r * a.ld;
    float raw[NPL];
#pragma unroll
    for (int j = 0; j < NPL; ++j) {
        const int c = lane + 64 * j;
        raw[j] = c < C ? row[c] : -INFINITY;
    }
    double lse = 0.0;
    if (a.logits) {                               // log-sum-exp over the row's columns, UNK excluded (fp64; beam_step's order)
        float m = -INFINITY;
#pragma unroll
        for (int j = 0; j < NPL; ++j) {
            const int c = lane + 64 * j;
            if (c < C && c != a.unk) m = fmaxf(m, raw[j]);
        }
        const double md = wave_max_d((double)m);
        double sm = 0.0;
#pragma unroll
        for (int j = 0; j < NPL; ++j) {
            const int c = lane + 64 * j;
            if (c < C && c != a.unk) sm += exp((double)raw[j] - md);
        }
        lse = md + log(wave_sum_d(sm));
    }
    const int skip_eos = p <= a.min_len ? a.eos : -1;
    float s[NPL];                                 // step scores (−inf off K0)
    u64 key[NPL];                                 // ≻ keys, 0 off the current candidate set
    int n0 = 0;
#pragma unroll
    for (int j = 0; j < NPL; ++j) {
        const int c = lane + 64 * j;
        float st;
        if (a.logits) st = (float)((double)raw[j] - lse);
        else st = raw[j] > 0.f ? (float)log((double)raw[j]) : -INFINITY;
        const bool cand = c < C && c != a.unk && c != skip_eos && st > -INFINITY;
        s[j] = cand ? st : -INFINITY;
        key[j] = cand ? ((u64)ord_key(raw[j]) << 12) | (u64)(kSampleColsMax - 1 - c) : 0ull;
        n0 += __popcll(__ballot(cand));
    }
    int ext, mod; float cu;
    int kept = 0;
    if (n0 == 0) {                                // no candidate: PAD, cum −inf, finished
        ext = a.pad; mod = a.pad; cu = -INFINITY;
    } else {
        // top-k: the k-th largest key t (count(key >= t) = k exactly, keys being distinct); K1 = keys >= t
        const int k = (a.topk <= 0 || a.topk >= n0) ? n0 : a.topk;
        if (k < n0) {
            u64 t = 0;
            for (int b = kKeyBits - 1; b >= 0; --b) {
                const u64 tt = t | (1ull << b);
                int n = 0;
                if constexpr (NPL <= 16) {        // ballots: counts in scalar registers
#pragma unroll
                    for (int j = 0; j < NPL; ++j) n += __popcll(__ballot(key[j] >= tt));
                } else {                          // (wider rows: per-lane counts, one wave sum — NPL ballots would not fit the SGPRs)
#pragma unroll
                    for (int j = 0; j < NPL; ++j) n += key[j] >= tt ? 1 : 0;
                    n = (int)wave_sum((float)n);
                }
                if (n >= k) t = tt;
            }
#pragma unroll
            for (int j = 0; j < NPL; ++j)
                if (key[j] < t) { key[j] = 0; s[j] = -INFINITY; }
        }
        // top-p: the largest t with S(t) = Σ_{K1, key >= t} w >= q·W; K2 = keys >= t (its first column alone has S = w_first = 1)
        if (a.topp > 0.0 && a.topp < 1.0) {
            float sf = -INFINITY;
#pragma unroll
            for (int j = 0; j < NPL; ++j) sf = fmaxf(sf, s[j]);
            const double zf = (double)wave_max(sf) / a.temp;     // z of the first column of K1 (z is monotone in the raw value)
            double w[NPL];
            double wl = 0.0;
#pragma unroll
            for (int j = 0; j < NPL; ++j) {
                w[j] = key[j] ? exp((double)s[j] / a.temp - zf) : 0.0;
                wl += w[j];
            }
            const double target = a.topp * wave_sum_dd(wl);
            u64 t = 0;
            for (int b = kKeyBits - 1; b >= 0; --b) {
                const u64 tt = t | (1ull << b);
                double sl = 0.0;
#pragma unroll
                for (int j = 0; j < NPL; ++j) sl += key[j] >= tt ? w[j] : 0.0;
                if (wave_sum_dd(sl) >= target) t = tt;
            }
#pragma unroll
            for (int j = 0; j < NPL; ++j)
                if (key[j] < t) key[j] = 0;
        }
        u64 alive = 0;                            // TRUNC: the survivors, bit j = column lane + 64·j
        if constexpr (TRUNC) {
#pragma unroll
            for (int j = 0; j < NPL; ++j)
                if (key[j]) alive |= 1ull << j;
            if (a.min_p > 0.0) {                      // min-p: w_c ≥ a (W is not needed)
                double w[NPL]; double zf;
                renorm<NPL>(s, alive, a.temp, w, zf);
                u64 keep = 0;
#pragma unroll
                for (int j = 0; j < NPL; ++j)
                    if (has_bit(alive, j) && w[j] >= a.min_p) keep |= 1ull << j;
                alive = keep;
            }
            if (a.typical_p > 0.0 && a.typical_p < 1.0) {
                double w[NPL]; double zf;
                const double W = renorm<NPL>(s, alive, a.temp, w, zf);
                const double lnW = log(W);
                const double H = entropy<NPL>(s, w, a.temp, zf, W, lnW);
                u64 zero = 0;                         // columns of the set with w = 0: d = +inf
#pragma unroll
                for (int j = 0; j < NPL; ++j) {
                    if (has_bit(alive, j) && w[j] == 0.0) zero |= 1ull << j;
                    w[j] = w[j] / W;                  // q from here on
                }
                // the bits of d_c, all ones off the set (above every probe).  They are held, in the wide variant too: recomputing d from s
                // and the row scalars at every probe, to spare the registers, spilled 320 bytes per lane where holding them fits in the
                // 512 registers (the resource report; look at it again after touching this stage)
                auto dbits = [&](int j) -> u64 {
                    if (!has_bit(alive, j)) return ~0ull;
                    const double d = has_bit(zero, j) ? (double)INFINITY : fabs(-(((double)s[j] / a.temp - zf) - lnW) - H);
                    return (u64)__double_as_longlong(d);
                };
                u64 d[NPL];
#pragma unroll
                for (int j = 0; j < NPL; ++j) d[j] = dbits(j);
                u64 t = 0;                            // the smallest t with Σ_{d ≤ t} q ≥ m; all ones when the whole sum stays below m
                for (int b = 62; b >= 0; --b) {
                    const u64 probe = t | ((1ull << b) - 1);
                    double sl = 0.0;
#pragma unroll
                    for (int j = 0; j < NPL; ++j) sl += d[j] <= probe ? w[j] : 0.0;
                    if (!(wave_sum_dd(sl) >= a.typical_p)) t |= 1ull << b;
                }
                u64 keep = 0;
#pragma unroll
                for (int j = 0; j < NPL; ++j)
                    if (d[j] <= t) keep |= 1ull << j;
                alive = keep;
            }
            if (a.epsilon > 0.0) {
                double w[NPL]; double zf;
                const double W = renorm<NPL>(s, alive, a.temp, w, zf);
                alive = keep_at_least<NPL>(row, lane, alive, w, W, a.epsilon);
            }
            if (a.eta > 0.0) {
                double w[NPL]; double zf;
                const double W = renorm<NPL>(s, alive, a.temp, w, zf);
                const double H = entropy<NPL>(s, w, a.temp, zf, W, log(W));
                alive = keep_at_least<NPL>(row, lane, alive, w, W, fmin(a.eta, sqrt(a.eta) * exp(-H)));
            }
            kept = __popcll(alive);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) kept += __shfl_xor(kept, o, 64);
        }
        // Gumbel-max over K2: the largest z_c + g_c, ties to the lower column; the step score travels with the winner
        const u64 seed = (u64)a.seed[0];
        double bk = -INFINITY; int bc = INT_MAX; float bs = 0.f;
#pragma unroll
        for (int j = 0; j < NPL; ++j) {
            if (TRUNC ? has_bit(alive, j) : key[j] != 0) {
                const int c = lane + 64 * j;
                const uint32_t h = svpc_hash32(seed, (uint32_t)a.pos, (u64)r * kSampleColsMax + (u64)c);
                const double u = ((double)h + 0.5) * (1.0 / 4294967296.0);
                const double g = (double)s[j] / a.temp - log(-log(u));
                if (g > bk || (g == bk && c < bc)) { bk = g; bc = c; bs = s[j]; }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ok = __shfl_xor(bk, o, 64);
            const int oc = __shfl_xor(bc, o, 64);
            const float os = __shfl_xor(bs, o, 64);
            if (ok > bk || (ok == bk && oc < bc)) { bk = ok; bc = oc; bs = os; }
        }
        ext = bc;
        mod = bc >= C - X ? a.unk : bc;
        cu = a.cum[r] + bs;
    }
    if (lane == 0) {
        a.cum[r] = cu;
        a.finished[r] = (n0 == 0 || ext == a.eos) ? 1 : 0;
        a.len[r] = p;
        a.next_ext[r] = ext; a.next_model[r] = mod;
        a.text_out[(size_t)r * a.ld_tok + p] = mod; a.ext_out[(size_t)r * a.ld_tok + p] = ext;
        if constexpr (TRUNC)
            if (a.kept_out) a.kept_out[r] = kept;
    }
}

// the seed of one sampling decode: src = (fixed, value); fixed != 0 → value, otherwise the decode's own seed word, which then advances (a
// Weyl step; the seed drawn from it is its splitmix64 image), so consecutive replays of a captured decode draw different streams
__global__ void sample_seed_kernel(const long long* __restrict__ src, long long* __restrict__ word, long long* __restrict__ used) {
    if (threadIdx.x != 0) return;
    if (src[0]) {
        used[0] = src[1];
        return;
    }
    u64 z = (u64)word[0] + 0x9E3779B97F4A7C15ull;
    word[0] = (long long)z;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    used[0] = (long long)(z >> 1);                // [0, 2^63), as a user's seed
}

}  // namespace

// the checks and the launch shared by the two entries
template <bool TRUNC>
int launch_sample_step(const char* name, const SampleArgs& a, int max_c, hipStream_t stream) {
    SVPC_REQUIRE(max_c >= 1 && max_c <= kSampleColsMax && max_c <= a.ld, "sample_step: row columns must be 1..4096 and within ld");
    SVPC_REQUIRE(a.pos >= 0 && a.pos + 1 < a.ld_tok, "sample_step: position pos + 1 must lie inside the id matrices");
    SVPC_REQUIRE(a.temp > 0.0 && a.temp <= 1.7976931348623157e308, "sample_step: temperature must be finite and > 0");
    SVPC_REQUIRE(a.topk >= 0 && a.topp >= 0.0 && a.topp <= 1.0, "sample_step: top-k >= 0 and top-p in [0, 1]");
    SVPC_REQUIRE(a.min_len >= 0 && a.min_len < a.ld_tok, "sample_step: min length must be 0..ld_tok-1");
    SVPC_REQUIRE(a.seed != nullptr, "sample_step: the seed word is required");
    const dim3 grid((a.n_rows + kSampleThreads / 64 - 1) / (kSampleThreads / 64)), block(kSampleThreads);
    if (max_c <= 1024) hipLaunchKernelGGL((sample_step_kernel<16, TRUNC>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((sample_step_kernel<64, TRUNC>), grid, block, 0, stream, a);
    return svpc_check_launch(name);
}

extern "C" {

int svpc_sample_step(const float* scores, int ld, const int* row_c, const int* row_x, int n_rows, int max_c, int pos, int logits, int unk,
                     int eos, int pad, double temp, int topk, double topp, int min_len, const long long* seed, float* cum, int* finished,
                     int* len, int* text_out, int* ext_out, int ld_tok, int* next_ext, int* next_model, hipStream_t stream) {
    if (n_rows == 0) return 0;
    const SampleArgs a{scores, ld, row_c, row_x, n_rows, pos, logits, unk, eos, pad, temp, topk, topp, min_len, seed, cum, finished, len,
                       text_out, ext_out, ld_tok, next_ext, next_model, 0.0, 0.0, 0.0, 0.0, nullptr};
    return launch_sample_step<false>("sample_step", a, max_c, stream);
}

int svpc_sample_step_trunc(const float* scores, int ld, const int* row_c, const int* row_x, int n_rows, int max_c, int pos, int logits,
                           int unk, int eos, int pad, double temp, int topk, double topp, int min_len, const long long* seed, float* cum,
                           int* finished, int* len, int* text_out, int* ext_out, int ld_tok, int* next_ext, int* next_model, double min_p,
                           double typical_p, double epsilon, double eta, int* kept_out, hipStream_t stream) {
    if (n_rows == 0) return 0;
    SVPC_REQUIRE(min_p >= 0.0 && min_p < 1.0 && typical_p >= 0.0 && typical_p <= 1.0 && epsilon >= 0.0 && epsilon < 1.0 && eta >= 0.0 &&
                     eta < 1.0, "sample_step_trunc: min-p, epsilon and eta in [0, 1), typical-p in [0, 1]");
    const SampleArgs a{scores, ld, row_c, row_x, n_rows, pos, logits, unk, eos, pad, temp, topk, topp, min_len, seed, cum, finished, len,
                       text_out, ext_out, ld_tok, next_ext, next_model, min_p, typical_p, epsilon, eta, kept_out};
    return launch_sample_step<true>("sample_step_trunc", a, max_c, stream);
}

int svpc_sample_seed(const long long* src, long long* word, long long* used, hipStream_t stream) {
    hipLaunchKernelGGL(sample_seed_kernel, dim3(1), dim3(64), 0, stream, src, word, used);
    return svpc_check_launch("sample_seed");
}

}  // extern "C"
