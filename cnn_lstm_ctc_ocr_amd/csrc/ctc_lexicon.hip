// Lexicon scoring (ocrk_ctc_lexicon_score): log p(word | logits) of every word
// of a list for every row of a batch -- the CTC forward sum of ctc.hip's loss
// (same extended-label lattice, same base-2 log-sum-exps), alpha only.
//
// The route this replaces replicates the [T, B, C] logits once per word and
// calls the loss on [T, B n_words, C]: every frame's log-sum-exp redone per
// word, a beta recursion and a lattice store nobody reads. Here:
//
// (1) lex_prep_kernel normalises each row's valid frames ONCE into a table of
//     log2 probabilities tab[b][t][c] in the workspace (a wave per frame), and,
//     in further workgroups of the same launch, checks every word once:
//     winfo[w] = the frames it needs (len + adjacent repeats), or -1 for a word
//     that is not scored (bad length / bad label value; word_status and the
//     status word's bit are set here).
// (2) lex_score_kernel: grid (chunks of LEX_WORDS words) x B, 1024 threads.
//     The workgroup copies its row's table into LDS (L C floats: 48 KB at the
//     serving shape 125 x 96), then each of its 16 waves takes the chunk's
//     words in turn and runs the alpha recursion alone, the lattice in R = 1,
//     2, 4 or 8 registers per lane chosen per word (S <= 64 shifts by DPP),
//     emissions gathered from the table one step ahead. Two words of at most
//     15 symbols (S <= 32) share a wave, one per 32-lane half: the recursion
//     is throughput-bound, so this nearly halves the time of a lexicon of
//     ordinary words (measured 327 -> 179 us at the serving shape, B = 64,
//     1000 words of 3..12 symbols). Only alpha[L-1][S-1] and alpha[L-1][S-2]
//     leave the wave. Nothing is stored per step and there is no barrier after
//     the table copy. A chunk with no feasible word (a narrow crop, seq_len 0)
//     skips the copy. When T C floats exceed LEX_LDS_MAX the waves gather from
//     the workspace table instead, up to four steps ahead.
// (3) lex_select_kernel, a workgroup per row: top_k rounds of "the best word
//     after the previous pick" in the order (logp descending, index
//     ascending), then the log-sum-exp of the finite scores with a fixed
//     summation tree. No floating-point atomics anywhere: a call's outputs are
//     reproducible bit for bit.
#include <climits>

#include "ctc_lattice.h"

#define LEX_THREADS 1024                 // measured 179 us at the serving shape, 1000 words; 186 at 512, 216 at 256
#define LEX_WAVES (LEX_THREADS / 64)
#define LEX_WORDS 64                     // words per workgroup: four per wave behind one table copy
#define LEX_PAIR_LEN 15                  // S = 2 len + 1 <= 32 states: two such words share a wave
#define LEX_LDS_MAX (112 * 1024)         // the table's LDS budget (the loss's lattice budget)
#define LEX_MAX_WORDS (1 << 20)
#define LEX_MAX_TOP 32
#define LEX_MAX_B 65535                  // rows ride the grid's y dimension
#define LEX_PREP_THREADS 256
#define LEX_SEL_THREADS 256

__global__ void __launch_bounds__(LEX_PREP_THREADS)
lex_prep_kernel(const float* __restrict__ logits, const int* __restrict__ seq_len, int T, int B, int C,
                const int* __restrict__ words, const int* __restrict__ word_len, int n_words, int max_word_len,
                float* __restrict__ tab, int* __restrict__ winfo, int* __restrict__ word_status,
                unsigned* __restrict__ status_word, int frame_blocks) {
    if ((int)blockIdx.x < frame_blocks) {
        // one wave per frame (b, t): tab = (logit - lse) * log2(e), the loss kernel's expressions
        constexpr int NQ = CTC_MAX_C / 64;
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        const int64_t f = (int64_t)blockIdx.x * (LEX_PREP_THREADS / 64) + wave;
        if (f >= (int64_t)B * T) return;
        const int b = (int)(f / T), t = (int)(f % T);
        if (t >= min(max(seq_len[b], 0), T)) return;       // frames past the sequence are never read
        const float* row = logits + ((size_t)t * B + b) * C;
        float v[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) v[q] = lane + 64 * q < C ? row[lane + 64 * q] : -INFINITY;
        float m = -INFINITY;
#pragma unroll
        for (int q = 0; q < NQ; ++q) m = fmaxf(m, v[q]);
        m = wave_max_dpp(m);
        float sum = 0.f;
#pragma unroll
        for (int q = 0; q < NQ; ++q)
            if (lane + 64 * q < C) sum += expf(v[q] - m);
        sum = wave_sum_dpp(sum);
        const float lse = m + logf(sum);
        float* out = tab + ((size_t)b * T + t) * C;
#pragma unroll
        for (int q = 0; q < NQ; ++q)
            if (lane + 64 * q < C) out[lane + 64 * q] = (v[q] - lse) * LOG2E_F;
        return;
    }
    // one thread per word: the loss's validation, with no row in sight. A bad length never indexes the
    // label row; a bad label value is only ever compared.
    const int w = ((int)blockIdx.x - frame_blocks) * LEX_PREP_THREADS + threadIdx.x;
    if (w >= n_words) return;
    const int len = word_len[w];
    int code = 0, req = -1;
    if (len < 0 || len > max_word_len) {
        code = 2;
    } else {
        const int* lab = words + (size_t)w * max_word_len;
        bool bad = false;
        int reps = 0, prev = -1;
        for (int i = 0; i < len; ++i) {
            const int v = lab[i];
            bad |= v < 0 || v >= C - 1;
            reps += i > 0 && v == prev;
            prev = v;
        }
        if (bad) code = 3;
        else req = len + reps;
    }
    winfo[w] = req;
    if (word_status) word_status[w] = code;
    if (code && status_word) __hip_atomic_fetch_or(status_word, 1u << code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ln p(word | the row's first L frames) for one word on one wave: ctc_alpha's
// recursion (state lane + 64 r in register r) without the lattice store. tab is
// the row's [L][C] log2-probability table (LDS, or the workspace when !LDS);
// the emissions of step t + D are read while step t computes. The caller has
// checked 0 <= len, len + repeats <= L, L >= 1 and the label values.
//
// PAIR (R = 1): two words of at most LEX_PAIR_LEN symbols (S <= 32) share the
// wave, one per 32-lane half; lab and len then differ between the halves, a
// lane's state is lane & 31, and state 0 of the upper half must not take lane
// 31's value from the whole-wave shift (two back is masked by skip already).
// The recursion is throughput-bound (four transcendentals per state and step,
// all SIMDs busy), so a half-empty wave is half the rate.
template <int R, bool LDS, bool PAIR = false>
__device__ __forceinline__ float lex_alpha(const float* __restrict__ tab, const int* __restrict__ lab, int len, int L,
                                           int C) {
    static_assert(!PAIR || R == 1, "paired words hold one register");
    // one step ahead covers the LDS latency; the workspace needs more (two at R = 8, where four would spill)
    constexpr int D = LDS ? 1 : R >= 8 ? 2 : 4;
    const int wlane = threadIdx.x & 63, lane = PAIR ? wlane & 31 : wlane, S = 2 * len + 1, blank = C - 1;
    int cls[R];
    bool skip[R];
    float a[R], en[D][R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int s = lane + 64 * r;
        const bool sym = s < S && (s & 1);                 // then s <= S - 2: label index s >> 1 < len
        const int c = sym ? lab[s >> 1] : blank;
        const int prev = (sym && s >= 3) ? lab[(s >> 1) - 1] : -1;
        cls[r] = c;
        skip[r] = sym && s >= 3 && c != prev;
        a[r] = (s < 2 && s < S) ? tab[c] : -INFINITY;
#pragma unroll
        for (int d = 0; d < D; ++d) en[d][r] = 1 + d < L ? tab[(1 + d) * C + c] : 0.f;
    }
    auto step = [&](const float* e) {
        float nxt[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float a1, a2;
            if constexpr (R == 1) {
                a1 = wave_shr1(a[0]);
                a2 = wave_shr1(a1);
                if constexpr (PAIR) a1 = lane == 0 ? -INFINITY : a1;
            } else {
                a1 = shift_up1(a, r, lane);
                a2 = shift_up2(a, r, lane);
            }
            a2 = skip[r] ? a2 : -INFINITY;
            nxt[r] = lse3b(a[r], a1, a2) + e[r];
        }
#pragma unroll
        for (int r = 0; r < R; ++r) a[r] = lane + 64 * r < S ? nxt[r] : -INFINITY;
    };
    // D whole steps per trip, the read ahead clamped to the last frame instead of predicated (ctc_viterbi's loop)
    int t0 = 1;
    for (; t0 + D <= L; t0 += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            float e[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                e[r] = en[d][r];
                en[d][r] = tab[min(t0 + d + D, L - 1) * C + cls[r]];
            }
            step(e);
        }
    }
#pragma unroll
    for (int d = 0; d < D; ++d)
        if (t0 + d < L) step(en[d]);
    // the two states a path may end in (S = 1: state -1 matches no register and stays -inf)
    const int s1 = S - 1, s2 = S - 2, half = PAIR ? wlane & 32 : 0;
    float x1 = -INFINITY, x2 = -INFINITY;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const float w1 = __shfl(a[r], half + (s1 & 63), 64), w2 = __shfl(a[r], (half + s2) & 63, 64);
        if ((s1 >> 6) == r) x1 = w1;
        if ((s2 >> 6) == r) x2 = w2;
    }
    return lse2b(x1, x2) * LN2_F;
}

template <bool LDS>
__global__ void __launch_bounds__(LEX_THREADS)
lex_score_kernel(const float* __restrict__ tab_g, const int* __restrict__ seq_len, int T, int C,
                 const int* __restrict__ words, const int* __restrict__ word_len, const int* __restrict__ winfo,
                 int n_words, int max_word_len, float* __restrict__ scores) {
    extern __shared__ float4 s_dyn4[];                     // LDS: the row's table, [L][C]
    const int b = blockIdx.y;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int L = min(max(seq_len[b], 0), T);
    const int w0 = blockIdx.x * LEX_WORDS;
    float* out = scores + (size_t)b * n_words;
    const float* tab_b = tab_g + (size_t)b * T * C;

    // a chunk with nothing to score (every word too long for this row, or not valid; L == 0) is all -inf
    bool feasible = false;
    if (threadIdx.x < LEX_WORDS && w0 + (int)threadIdx.x < n_words) {
        const int req = winfo[w0 + threadIdx.x];
        feasible = L > 0 && req >= 0 && req <= L;
    }
    if (!__syncthreads_or(feasible)) {
        if (threadIdx.x < LEX_WORDS && w0 + (int)threadIdx.x < n_words) out[w0 + threadIdx.x] = -INFINITY;
        return;
    }
    const float* tab = tab_b;
    if constexpr (LDS) {
        const int n = L * C;                               // <= T C floats = the launch's dynamic LDS
        if ((C & 3) == 0) {                                // rows of whole float4s: tab_b is 16-B aligned
            const float4* src = reinterpret_cast<const float4*>(tab_b);
            for (int i = threadIdx.x; i < (n >> 2); i += LEX_THREADS) s_dyn4[i] = src[i];
        } else {
            float* dst = reinterpret_cast<float*>(s_dyn4);
            for (int i = threadIdx.x; i < n; i += LEX_THREADS) dst[i] = tab_b[i];
        }
        __syncthreads();
        tab = reinterpret_cast<const float*>(s_dyn4);
    }
    // a wave takes the chunk's words wi and wi + LEX_WAVES together: both on one pass of the recursion when
    // both are to be scored and short enough for half a wave each, else one after the other
    for (int wi = wave; wi < LEX_WORDS; wi += 2 * LEX_WAVES) {
        int w[2], len[2];                                  // wave-uniform
        bool ok[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            w[h] = w0 + wi + h * LEX_WAVES;
            const int req = w[h] < n_words ? __builtin_amdgcn_readfirstlane(winfo[w[h]]) : -1;
            ok[h] = req >= 0 && req <= L;
            len[h] = ok[h] ? __builtin_amdgcn_readfirstlane(word_len[w[h]]) : 0;   // in [0, max_word_len]: req >= 0
        }
        if (w[0] >= n_words) break;
        if (ok[0] && ok[1] && len[0] <= LEX_PAIR_LEN && len[1] <= LEX_PAIR_LEN) {
            const int h = lane >> 5;
            const float lp = lex_alpha<1, LDS, true>(tab, words + (size_t)(h ? w[1] : w[0]) * max_word_len,
                                                     h ? len[1] : len[0], L, C);
            if ((lane & 31) == 0) out[h ? w[1] : w[0]] = lp;
            continue;
        }
#pragma unroll 1
        for (int h = 0; h < 2; ++h) {
            const int wh = h ? w[1] : w[0], n = h ? len[1] : len[0];
            if (wh >= n_words) break;
            float lp = -INFINITY;
            if (h ? ok[1] : ok[0]) {
                const int* lab = words + (size_t)wh * max_word_len;
                const int S = 2 * n + 1;
                if (S <= 64) lp = lex_alpha<1, LDS>(tab, lab, n, L, C);
                else if (S <= 128) lp = lex_alpha<2, LDS>(tab, lab, n, L, C);
                else if (S <= 256) lp = lex_alpha<4, LDS>(tab, lab, n, L, C);
                else lp = lex_alpha<8, LDS>(tab, lab, n, L, C);
            }
            if (lane == 0) out[wh] = lp;
        }
    }
}

// (value, index) of the better of two candidates: larger score, then smaller index
__device__ __forceinline__ void lex_better(float& bv, int& bi, float ov, int oi) {
    if (ov > bv || (ov == bv && oi < bi)) {
        bv = ov;
        bi = oi;
    }
}

__global__ void __launch_bounds__(LEX_SEL_THREADS)
lex_select_kernel(const float* __restrict__ scores, int n_words, int top_k, int* __restrict__ top_idx,
                  float* __restrict__ top_logp, float* __restrict__ log_norm) {
    constexpr int NW = LEX_SEL_THREADS / 64;
    __shared__ float s_v[NW], s_sum[NW], s_bv;
    __shared__ int s_i[NW], s_bi;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const float* row = scores + (size_t)b * n_words;
    float pv = INFINITY, best = -INFINITY;                 // the previous pick; the row's best score
    int pi = -1, j = 0;
    for (; j < top_k; ++j) {
        float bv = -INFINITY;
        int bi = INT_MAX;
        for (int i = tid; i < n_words; i += LEX_SEL_THREADS) {
            const float v = row[i];
            const bool after = v < pv || (v == pv && i > pi);
            if (after && v > bv) {                         // i ascends: the first of equal scores stays
                bv = v;
                bi = i;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) lex_better(bv, bi, __shfl_xor(bv, o, 64), __shfl_xor(bi, o, 64));
        if (lane == 0) {
            s_v[wave] = bv;
            s_i[wave] = bi;
        }
        __syncthreads();
        if (tid == 0) {
            for (int k = 1; k < NW; ++k) lex_better(bv, bi, s_v[k], s_i[k]);
            s_bv = bv;
            s_bi = bi;
        }
        __syncthreads();
        pv = s_bv;
        pi = s_bi;
        if (!(pv > -INFINITY)) break;                      // no feasible word is left (block-uniform)
        if (j == 0) best = pv;
        if (tid == 0) {
            top_idx[(size_t)b * top_k + j] = pi;
            top_logp[(size_t)b * top_k + j] = pv;
        }
    }
    for (int k = j + tid; k < top_k; k += LEX_SEL_THREADS) {
        top_idx[(size_t)b * top_k + k] = -1;
        top_logp[(size_t)b * top_k + k] = -INFINITY;
    }
    if (!log_norm) return;
    if (!(best > -INFINITY)) {
        if (tid == 0) log_norm[b] = -INFINITY;
        return;
    }
    // strided partial sums, a butterfly per wave, the waves in order: one fixed tree
    float acc = 0.f;
    for (int i = tid; i < n_words; i += LEX_SEL_THREADS) {
        const float v = row[i];
        if (v > -INFINITY) acc += expf(v - best);
    }
    acc = wave_sum(acc);
    if (lane == 0) s_sum[wave] = acc;
    __syncthreads();
    if (tid == 0) {
        float tot = 0.f;
        for (int k = 0; k < NW; ++k) tot += s_sum[k];
        log_norm[b] = best + logf(tot);
    }
}

// ------------------------------------------------------------------- C ABI
static size_t lex_round16(size_t n) { return (n + 15) & ~(size_t)15; }
static bool lex_sizes_ok(int T, int B, int C, int n_words, int max_word_len) {
    return T > 0 && T <= CTC_MAX_T && B >= 0 && B <= LEX_MAX_B && C >= 2 && C <= CTC_MAX_C && n_words >= 1 &&
           n_words <= LEX_MAX_WORDS && max_word_len >= 0 && 2 * max_word_len + 1 <= 64 * CTC_MAX_R;
}
static size_t lex_tab_bytes(int T, int B, int C) { return lex_round16((size_t)B * T * C * sizeof(float)); }
static size_t lex_winfo_bytes(int n_words) { return lex_round16((size_t)n_words * sizeof(int)); }

extern "C" size_t ocrk_ctc_lexicon_workspace_size(int T, int B, int C, int n_words, int max_word_len) {
    if (!lex_sizes_ok(T, B, C, n_words, max_word_len)) return 0;
    return lex_tab_bytes(T, B, C) + lex_winfo_bytes(n_words) + lex_round16((size_t)B * n_words * sizeof(float));
}

extern "C" int ocrk_ctc_lexicon_score(const float* logits, const int* seq_len, int T, int B, int C, const int* words,
                                      const int* word_len, int n_words, int max_word_len, int top_k, float* logp,
                                      int* top_idx, float* top_logp, float* log_norm, int* word_status,
                                      uint32_t* status_word, void* ws, size_t ws_bytes, void* stream) {
    OCRK_REQUIRE(T > 0 && T <= CTC_MAX_T, "ocrk_ctc_lexicon_score: T=%d out of range (1..%d)", T, CTC_MAX_T);
    OCRK_REQUIRE(B >= 0 && B <= LEX_MAX_B && C >= 2 && C <= CTC_MAX_C, "ocrk_ctc_lexicon_score: bad B=%d / C=%d", B,
                 C);
    OCRK_REQUIRE(n_words >= 1 && n_words <= LEX_MAX_WORDS, "ocrk_ctc_lexicon_score: n_words=%d out of range (1..%d)",
                 n_words, LEX_MAX_WORDS);
    OCRK_REQUIRE(max_word_len >= 0 && 2 * max_word_len + 1 <= 64 * CTC_MAX_R,
                 "ocrk_ctc_lexicon_score: max_word_len=%d too long (<= %d)", max_word_len, (64 * CTC_MAX_R - 1) / 2);
    OCRK_REQUIRE(top_k >= 1 && top_k <= LEX_MAX_TOP, "ocrk_ctc_lexicon_score: top_k=%d out of range (1..%d)", top_k,
                 LEX_MAX_TOP);
    OCRK_REQUIRE(ws_bytes >= ocrk_ctc_lexicon_workspace_size(T, B, C, n_words, max_word_len),
                 "ocrk_ctc_lexicon_score: workspace too small");
    if (B == 0) return OCRK_OK;
    OCRK_REQUIRE(logits && seq_len && word_len && (words || max_word_len == 0) && top_idx && top_logp && ws,
                 "ocrk_ctc_lexicon_score: null pointer");
    OCRK_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "ocrk_ctc_lexicon_score: ws must be 16-B aligned");
    hipStream_t s = ocrk::as_stream(stream);
    unsigned char* base = static_cast<unsigned char*>(ws);
    float* tab = reinterpret_cast<float*>(base);
    int* winfo = reinterpret_cast<int*>(base + lex_tab_bytes(T, B, C));
    float* scores = logp ? logp : reinterpret_cast<float*>(base + lex_tab_bytes(T, B, C) + lex_winfo_bytes(n_words));

    const int frame_blocks = (int)ocrk::cdiv((int64_t)B * T, LEX_PREP_THREADS / 64);
    const int word_blocks = (int)ocrk::cdiv(n_words, LEX_PREP_THREADS);
    lex_prep_kernel<<<frame_blocks + word_blocks, LEX_PREP_THREADS, 0, s>>>(
        logits, seq_len, T, B, C, words, word_len, n_words, max_word_len, tab, winfo, word_status, status_word,
        frame_blocks);

    const dim3 grid((unsigned)ocrk::cdiv(n_words, LEX_WORDS), (unsigned)B);
    const size_t dyn = (size_t)T * C * sizeof(float);
    if (dyn <= LEX_LDS_MAX && ocrk::opt(ocrk::OPT_CTC_LDS) != 0) {      // 0: the table stays in the workspace
        static ocrk::DeviceOnce attr;
        ocrk::set_dyn_lds(attr, reinterpret_cast<const void*>(&lex_score_kernel<true>), LEX_LDS_MAX);
        lex_score_kernel<true><<<grid, LEX_THREADS, dyn, s>>>(tab, seq_len, T, C, words, word_len, winfo, n_words,
                                                             max_word_len, scores);
    } else {
        lex_score_kernel<false><<<grid, LEX_THREADS, 0, s>>>(tab, seq_len, T, C, words, word_len, winfo, n_words,
                                                             max_word_len, scores);
    }
    lex_select_kernel<<<B, LEX_SEL_THREADS, 0, s>>>(scores, n_words, top_k, top_idx, top_logp, log_norm);
    return ocrk::launch_status("ocrk_ctc_lexicon_score");
}
