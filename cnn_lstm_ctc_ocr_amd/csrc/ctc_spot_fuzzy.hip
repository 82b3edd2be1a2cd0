// Error-tolerant keyword spotting on the CTC lattice (ocrk_ctc_spot_fuzzy): for
// every row of a batch and every keyword of a list, the best path INSIDE the row
// that spells the keyword with at most err[k] <= 2 edits -- a substituted symbol,
// an inserted one, a deleted inner one -- as a likelihood ratio against the
// greedy path, the number of edits it used and its frames. The exact spotter
// (ctc_spot.hip) scores "T0TAL" and "TOTL" against TOTAL as badly as an
// unrelated word; here they are one edit away.
//
// include/ocrk.h states the recursion and its tie order; tests/ctc_spot_fuzzy_ref.py
// restates it in NumPy and the device is compared with that bit for bit. In short:
// layers e = 0..err of the exact spotter's chain M[e][s] (S = 2 n - 1 states, the
// same emissions), and for e >= 1 a wild state W[e][s] on every lane that emits
// nb(t), the frame's best non-blank rel: on an even lane it stands for symbol s/2
// (a substitution), on an odd lane it is one extra symbol (an insertion). A wild
// run lasts while the frame's best non-blank class a(t) stays the same -- exactly
// one character -- and may not touch a neighbour of that class without a blank.
// A deletion is the edge from M[e-1][s-3] or M[e-1][s-4] into M[e][s]. Every edge
// that raises e costs edit_cost, one float32 subtraction.
//
// (1) fuzzy_prep_kernel: ctc_spot.hip's prep launch with two additions. The wave
//     that writes a frame's rel row also writes (nb(t), a(t)) into nba[b][t];
//     the thread that checks a keyword also checks its budget, and kinfo[k] is a
//     lower bound of the frames the keyword needs (the exact one for budget 0).
// (2) fuzzy_score_kernel: ctc_spot.hip's layout -- grid (chunks of SPOT_KW = 16
//     keywords) x B, 512 threads, the row's table in LDS with (nb, a) behind it,
//     a pair of adjacent keywords per wave, two of at most 16 symbols side by
//     side, state s on lane s. A wave whose keywords both have budget 0 runs the
//     exact spotter's recursion itself (spot_best, ctc_lattice.h). Otherwise
//     fuzzy_best<E> holds the E + 1 chains and E wild rows with their start
//     frames in registers (at most 5 + 5) and moves them with whole-wave DPP
//     shifts, up to four lanes back for the deletions; E is the larger budget of
//     the wave's two keywords, and a lane whose keyword has a smaller one keeps
//     the layers above it at -inf. The next step's emission and (nb, a) are read
//     one step ahead (four on the workspace route). Nothing is stored per step.
// No floating-point atomics: a call's outputs are reproducible bit for bit.
#include "ctc_lattice.h"

#define FUZZY_MAX_ERR 2

// The frame part of the prep launch: ctc_rel_frame's rel row, and behind it the frame's best non-blank rel
// and the lowest class that attains it (compared on the rounded rel values, as the definition has it).
template <int THREADS>
__device__ __forceinline__ void fuzzy_rel_frame(const float* __restrict__ logits, const int* __restrict__ seq_len,
                                                int T, int B, int C, float* __restrict__ tab,
                                                float2* __restrict__ nba) {
    constexpr int NQ = CTC_MAX_C / 64;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t f = (int64_t)blockIdx.x * (THREADS / 64) + wave;
    if (f >= (int64_t)B * T) return;
    const int b = (int)(f / T), t = (int)(f % T);
    if (t >= min(max(seq_len[b], 0), T)) return;           // frames past the sequence are never read
    const float* row = logits + ((size_t)t * B + b) * C;
    float v[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) v[q] = lane + 64 * q < C ? row[lane + 64 * q] : -INFINITY;
    float m = -INFINITY;
#pragma unroll
    for (int q = 0; q < NQ; ++q) m = fmaxf(m, v[q]);
    m = wave_max_dpp(m);
    float* out = tab + ((size_t)b * T + t) * C;
    float nb = -INFINITY;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        v[q] -= m;
        if (lane + 64 * q < C) out[lane + 64 * q] = v[q];
        if (lane + 64 * q < C - 1) nb = fmaxf(nb, v[q]);
    }
    nb = wave_max_dpp(nb);
    int a = -1;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const unsigned long long hit = __builtin_amdgcn_ballot_w64(lane + 64 * q < C - 1 && v[q] == nb);
        if (a < 0 && hit) a = 64 * q + __builtin_ctzll(hit);
    }
    if (lane == 0) nba[(size_t)b * T + t] = make_float2(nb, __int_as_float(max(a, 0)));
}

__global__ void __launch_bounds__(SPOT_PREP_THREADS)
fuzzy_prep_kernel(const float* __restrict__ logits, const int* __restrict__ seq_len, int T, int B, int C,
                  const int* __restrict__ kw, const int* __restrict__ kw_alt, const int* __restrict__ kw_len,
                  const int* __restrict__ kw_err, int n_kw, int max_kw_len, float* __restrict__ tab,
                  float2* __restrict__ nba, int* __restrict__ kinfo, int* __restrict__ kw_status,
                  unsigned* __restrict__ status_word, int frame_blocks) {
    if ((int)blockIdx.x < frame_blocks) {
        fuzzy_rel_frame<SPOT_PREP_THREADS>(logits, seq_len, T, B, C, tab, nba);
        return;
    }
    // one thread per keyword, with no row in sight (spot_check_keyword, ctc_lattice.h), then its budget
    const int k = ((int)blockIdx.x - frame_blocks) * SPOT_PREP_THREADS + threadIdx.x;
    if (k >= n_kw) return;
    int req;
    int code = spot_check_keyword(kw, kw_alt, kw_len, k, max_kw_len, C, req);
    if (!code) {
        const int len = kw_len[k], err = kw_err[k];
        if (err < 0 || err > min(FUZZY_MAX_ERR, len - 1)) {
            code = 2;
            req = -1;
        } else if (err > 0) {
            req = len - err;                               // a lower bound: every symbol left needs a frame
        }
    }
    kinfo[k] = req;
    if (kw_status) kw_status[k] = code;
    if (code && status_word) __hip_atomic_fetch_or(status_word, 1u << code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The best path of one keyword with at most err edits on one wave (PAIR: of two keywords, one per 32-lane half;
// lab, alt, len and err then differ between the halves). E >= 1 is the larger budget of the wave: the layers
// above a lane's own err stay at -inf. tab and nba are the row's [L][C] table of rel and its [L] pairs
// (nb, a); len is 0 for a keyword that is not to be scored here. Every candidate that crosses lanes names
// its least lane in a lane mask, so in a pair the upper half never takes the lower half's values from the
// whole-wave shifts. The result is returned on every lane of the keyword's half.
template <bool LDS, bool ALT, bool PAIR, int E>
__device__ __forceinline__ void fuzzy_best(const float* __restrict__ tab, const float2* __restrict__ nba,
                                           const int* __restrict__ lab, const int* __restrict__ alt, int len,
                                           int err, float cost, int L, int C, float& score, int& first, int& end,
                                           int& errors) {
    constexpr int D = LDS ? 1 : 4;                         // one step ahead covers the LDS latency
    const int wlane = threadIdx.x & 63, s = PAIR ? wlane & 31 : wlane, S = 2 * len - 1;
    const bool active = s < S, sym = active && !(s & 1);   // then label index s >> 1 < len
    const int i = s >> 1;
    // the lane's own set {c0, c1} (the blank twice on an odd lane) and the set {p0, p1} of the symbol before
    // the lane, index (s - 1) >> 1 (nothing at s = 0: -1 matches no class)
    const int c0 = sym ? lab[i] : C - 1;
    int c1 = c0, p0 = -1, p1 = -1;
    if constexpr (ALT) {
        if (sym && alt[i] >= 0) c1 = alt[i];
    }
    if (active && s >= 1) {
        p0 = p1 = lab[(s - 1) >> 1];
        if constexpr (ALT) {
            if (alt[(s - 1) >> 1] >= 0) p1 = alt[(s - 1) >> 1];
        }
    }
    auto disjoint = [&](int j) {                           // set(i) and set(j) share no class (j < i)
        const int l = lab[j];
        bool d = c0 != l && c1 != l;
        if constexpr (ALT) {
            const int a = alt[j];
            d = d && (a < 0 || (c0 != a && c1 != a));
        }
        return d;
    };
    const bool odd = active && (s & 1);
    const bool ge1 = active && s >= 1, even2 = sym && s >= 2, even4 = sym && s >= 4;
    const bool skip = even2 && disjoint(i - 1), skip4 = even4 && disjoint(i - 2);
    bool act[E + 1];
#pragma unroll
    for (int e = 0; e <= E; ++e) act[e] = active && e <= err;

    auto emit = [&](int t) {
        const float e = tab[t * C + c0];
        if constexpr (ALT) return fmaxf(e, tab[t * C + c1]);
        return e;
    };
    float M[E + 1], W[E + 1], best_v = -INFINITY, en[D];
    int Ms[E + 1], Ws[E + 1], best_f = -1, best_e = -1, best_n = -1;
    float2 wn[D];
#pragma unroll
    for (int e = 0; e <= E; ++e) {
        M[e] = W[e] = -INFINITY;
        Ms[e] = Ws[e] = -1;
    }
#pragma unroll
    for (int d = 0; d < D; ++d) {
        en[d] = emit(min(d, L - 1));
        wn[d] = nba[min(d, L - 1)];
    }
    int a_prev = -1;                                       // a(t - 1); no class before frame 0
    bool own_prev = true;                                  // a(t - 1) is outside the lane's own set
    auto take = [](bool ok, float v, int vs, float& b, int& bs) {
        if (ok && v > b) {                                 // only if strictly greater
            b = v;
            bs = vs;
        }
    };
    auto step = [&](float e_own, float2 w, int t) {
        const float nb = w.x;
        const int a = __float_as_int(w.y);
        const bool same = a == a_prev;                     // false at t = 0
        const bool pne = a != p0 && a != p1;               // a(t) is outside the set of the symbol before the lane
        // the values of frame t - 1 from one to four lanes back
        float m1[E + 1], m2[E + 1], m3[E], m4[E], w1[E + 1], w2[E + 1];
        int ms1[E + 1], ms2[E + 1], ms3[E], ms4[E], ws1[E + 1], ws2[E + 1];
#pragma unroll
        for (int e = 0; e <= E; ++e) {
            m1[e] = wave_shr1(M[e]);
            ms1[e] = spot_shr1(Ms[e]);
            m2[e] = wave_shr1(m1[e]);
            ms2[e] = spot_shr1(ms1[e]);
            if (e < E) {
                m3[e] = wave_shr1(m2[e]);
                ms3[e] = spot_shr1(ms2[e]);
                m4[e] = wave_shr1(m3[e]);
                ms4[e] = spot_shr1(ms3[e]);
            }
            if (e >= 1) {
                w1[e] = wave_shr1(W[e]);
                ws1[e] = spot_shr1(Ws[e]);
                w2[e] = wave_shr1(w1[e]);
                ws2[e] = spot_shr1(ws1[e]);
            }
        }
        // the layers from the top down: layer e reads frame t - 1 of layers e and e - 1 only
#pragma unroll
        for (int e = E; e >= 1; --e) {
            float b = M[e];                                // stay
            int bs = Ms[e];
            take(ge1, m1[e], ms1[e], b, bs);               // one back
            take(skip, m2[e], ms2[e], b, bs);              // two back, where the two symbol sets are disjoint
            take(odd, W[e], Ws[e], b, bs);                 // the blank after an inserted symbol
            take(odd || (even2 && own_prev), w1[e], ws1[e], b, bs);
            take(even2 && own_prev, w2[e], ws2[e], b, bs);
            take(even4, m3[e - 1] - cost, ms3[e - 1], b, bs);   // symbol i - 1 deleted, after a blank
            take(skip4, m4[e - 1] - cost, ms4[e - 1], b, bs);   // and straight from symbol i - 2
            float wb = same ? W[e] : -INFINITY;            // the wild run goes on while its class does
            int wbs = same ? Ws[e] : -1;
            take(odd, M[e - 1] - cost, Ms[e - 1], wb, wbs);
            take(sym ? s >= 1 : (odd && pne), m1[e - 1] - cost, ms1[e - 1], wb, wbs);
            take(even2 && pne, m2[e - 1] - cost, ms2[e - 1], wb, wbs);
            if (e == 1) take(s == 0, 0.f - cost, t, wb, wbs);
            if (e == 2) take(ge1 && !same, w1[1] - cost, ws1[1], wb, wbs);
            M[e] = act[e] ? b + e_own : -INFINITY;
            Ms[e] = bs;
            W[e] = act[e] ? wb + nb : -INFINITY;
            Ws[e] = wbs;
        }
        {
            float b = M[0];
            int bs = Ms[0];
            take(ge1, m1[0], ms1[0], b, bs);
            take(skip, m2[0], ms2[0], b, bs);
            take(s == 0, 0.f, t, b, bs);                   // entry: the filler before the hit scores 0
            M[0] = active ? b + e_own : -INFINITY;
            Ms[0] = bs;
        }
        a_prev = a;
        own_prev = a != c0 && a != c1;
        // read on the lane of state S - 1 only: the layers ascending, the chain before the wild
#pragma unroll
        for (int e = 0; e <= E; ++e) {
            if (M[e] > best_v) {
                best_v = M[e];
                best_f = Ms[e];
                best_e = t + 1;
                best_n = e;
            }
            if (e >= 1 && W[e] > best_v) {
                best_v = W[e];
                best_f = Ws[e];
                best_e = t + 1;
                best_n = e;
            }
        }
    };
    // D whole steps per trip, the read ahead clamped to the last frame instead of predicated
    int t0 = 0;
    for (; t0 + D <= L; t0 += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const float e = en[d];
            const float2 w = wn[d];
            en[d] = emit(min(t0 + d + D, L - 1));
            wn[d] = nba[min(t0 + d + D, L - 1)];
            step(e, w, t0 + d);
        }
    }
#pragma unroll
    for (int d = 0; d < D; ++d)
        if (t0 + d < L) step(en[d], wn[d], t0 + d);
    const int src = (PAIR ? wlane & 32 : 0) + max(S - 1, 0);
    score = __shfl(best_v, src, 64);
    first = __shfl(best_f, src, 64);
    end = __shfl(best_e, src, 64);
    errors = __shfl(best_n, src, 64);
}

// One keyword (PAIR: one per half) by the recursion its wave needs: the exact spotter's for budget 0.
template <bool LDS, bool ALT, bool PAIR>
__device__ __forceinline__ void fuzzy_dispatch(int emax, const float* __restrict__ tab,
                                               const float2* __restrict__ nba, const int* __restrict__ lab,
                                               const int* __restrict__ alt, int len, int err, float cost, int L,
                                               int C, float& v, int& f, int& e, int& n) {
    if (emax == 0) {
        spot_best<LDS, ALT, PAIR, false>(tab, lab, alt, len, L, C, nullptr, v, f, e);
        n = e >= 0 ? 0 : -1;
    } else if (emax == 1) {
        fuzzy_best<LDS, ALT, PAIR, 1>(tab, nba, lab, alt, len, err, cost, L, C, v, f, e, n);
    } else {
        fuzzy_best<LDS, ALT, PAIR, 2>(tab, nba, lab, alt, len, err, cost, L, C, v, f, e, n);
    }
}

// grid (chunks of SPOT_KW keywords) x B, SPOT_THREADS threads; when LDS, lds_nba * 4 + 8 T bytes of dynamic
// LDS: the row's table [L][C], and from float lds_nba on its (nb, a) pairs [L].
template <bool LDS, bool ALT>
__global__ void __launch_bounds__(SPOT_THREADS)
fuzzy_score_kernel(const float* __restrict__ tab_g, const float2* __restrict__ nba_g, const int* __restrict__ seq_len,
                   int T, int C, int lds_nba, const int* __restrict__ kw, const int* __restrict__ kw_alt,
                   const int* __restrict__ kw_len, const int* __restrict__ kw_err, const int* __restrict__ kinfo,
                   int n_kw, int max_kw_len, float cost, float* __restrict__ score, int* __restrict__ span,
                   int* __restrict__ errors) {
    extern __shared__ float4 s_dyn4[];
    const int b = blockIdx.y;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int L = min(max(seq_len[b], 0), T);
    const int k0 = blockIdx.x * SPOT_KW;
    float* out_v = score + (size_t)b * n_kw;
    int2* out_s = reinterpret_cast<int2*>(span) + (size_t)b * n_kw;
    int* out_n = errors + (size_t)b * n_kw;
    const float* tab_b = tab_g + (size_t)b * T * C;
    const float2* nba_b = nba_g + (size_t)b * T;

    // a chunk with nothing to score (every keyword too long for this row, or not valid; L == 0)
    bool feasible = false;
    if (threadIdx.x < SPOT_KW && k0 + (int)threadIdx.x < n_kw) {
        const int req = kinfo[k0 + threadIdx.x];
        feasible = req >= 0 && req <= L;                   // req >= 1: never with L == 0
    }
    if (!__syncthreads_or(feasible)) {
        if (threadIdx.x < SPOT_KW && k0 + (int)threadIdx.x < n_kw) {
            out_v[k0 + threadIdx.x] = -INFINITY;
            out_s[k0 + threadIdx.x] = make_int2(-1, -1);
            out_n[k0 + threadIdx.x] = -1;
        }
        return;
    }
    const float* tab = tab_b;
    const float2* nba = nba_b;
    if constexpr (LDS) {
        ctc_tab_to_lds<SPOT_THREADS>(tab_b, s_dyn4, L, C, C);   // <= T C floats, below lds_nba
        float2* dst = reinterpret_cast<float2*>(reinterpret_cast<float*>(s_dyn4) + lds_nba);
        for (int t = threadIdx.x; t < L; t += SPOT_THREADS) dst[t] = nba_b[t];
        __syncthreads();
        tab = reinterpret_cast<const float*>(s_dyn4);
        nba = dst;
    }
    // a wave takes the adjacent keywords 2 p and 2 p + 1 together: both on one pass of the recursion when
    // neither needs more than half a wave, else one after the other
    for (int p = wave; 2 * p < SPOT_KW; p += SPOT_WAVES) {
        int k[2], len[2], err[2];                          // wave-uniform
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            k[h] = k0 + 2 * p + h;
            const int req = k[h] < n_kw ? __builtin_amdgcn_readfirstlane(kinfo[k[h]]) : -1;
            // scored: then the length is in [1, min(32, max_kw_len)] and the budget in [0, min(2, len - 1)]
            const bool scored = req >= 0 && req <= L;
            len[h] = scored ? __builtin_amdgcn_readfirstlane(kw_len[k[h]]) : 0;
            err[h] = scored ? __builtin_amdgcn_readfirstlane(kw_err[k[h]]) : 0;
        }
        if (k[0] >= n_kw) break;
        if (len[0] <= SPOT_PAIR_LEN && len[1] <= SPOT_PAIR_LEN) {
            const int h = lane >> 5, kh = h ? k[1] : k[0];
            float v = -INFINITY;
            int f = -1, e = -1, n = -1;
            if (len[0] | len[1])
                fuzzy_dispatch<LDS, ALT, true>(max(err[0], err[1]), tab, nba,
                                               kw + (size_t)min(kh, n_kw - 1) * max_kw_len,
                                               ALT ? kw_alt + (size_t)min(kh, n_kw - 1) * max_kw_len : nullptr,
                                               h ? len[1] : len[0], h ? err[1] : err[0], cost, L, C, v, f, e, n);
            if ((lane & 31) == 0 && kh < n_kw) {
                out_v[kh] = v;
                out_s[kh] = make_int2(f, e);
                out_n[kh] = n;
            }
            continue;
        }
#pragma unroll 1
        for (int h = 0; h < 2; ++h) {
            const int kh = h ? k[1] : k[0], n_sym = h ? len[1] : len[0], eh = h ? err[1] : err[0];
            if (kh >= n_kw) break;
            float v = -INFINITY;
            int f = -1, e = -1, n = -1;
            if (n_sym)
                fuzzy_dispatch<LDS, ALT, false>(eh, tab, nba, kw + (size_t)kh * max_kw_len,
                                                ALT ? kw_alt + (size_t)kh * max_kw_len : nullptr, n_sym, eh, cost, L,
                                                C, v, f, e, n);
            if (lane == 0) {
                out_v[kh] = v;
                out_s[kh] = make_int2(f, e);
                out_n[kh] = n;
            }
        }
    }
}

// ------------------------------------------------------------------- C ABI
static size_t fuzzy_round16(size_t n) { return (n + 15) & ~(size_t)15; }
static bool fuzzy_sizes_ok(int T, int B, int C, int n_kw, int max_kw_len) {
    return T > 0 && T <= CTC_MAX_T && B >= 0 && B <= SPOT_MAX_B && C >= 2 && C <= CTC_MAX_C && n_kw >= 1 &&
           n_kw <= SPOT_MAX_KW && max_kw_len >= 1 && max_kw_len <= SPOT_MAX_WIDTH;
}
static size_t fuzzy_tab_bytes(int T, int B, int C) { return fuzzy_round16((size_t)B * T * C * sizeof(float)); }
static size_t fuzzy_nba_bytes(int T, int B) { return fuzzy_round16((size_t)B * T * sizeof(float2)); }

extern "C" size_t ocrk_ctc_spot_fuzzy_workspace_size(int T, int B, int C, int n_kw, int max_kw_len) {
    if (!fuzzy_sizes_ok(T, B, C, n_kw, max_kw_len)) return 0;
    return fuzzy_tab_bytes(T, B, C) + fuzzy_nba_bytes(T, B) + fuzzy_round16((size_t)n_kw * sizeof(int));
}

template <bool LDS, bool ALT>
static void fuzzy_launch(dim3 grid, size_t dyn, hipStream_t s, const float* tab, const float2* nba,
                         const int* seq_len, int T, int C, int lds_nba, const int* kw, const int* kw_alt,
                         const int* kw_len, const int* kw_err, const int* kinfo, int n_kw, int max_kw_len,
                         float cost, float* score, int* span, int* errors) {
    if constexpr (LDS) {
        static ocrk::DeviceOnce attr;
        ocrk::set_dyn_lds(attr, reinterpret_cast<const void*>(&fuzzy_score_kernel<true, ALT>), SPOT_LDS_MAX);
    }
    fuzzy_score_kernel<LDS, ALT><<<grid, SPOT_THREADS, dyn, s>>>(tab, nba, seq_len, T, C, lds_nba, kw, kw_alt, kw_len,
                                                                kw_err, kinfo, n_kw, max_kw_len, cost, score, span,
                                                                errors);
}

extern "C" int ocrk_ctc_spot_fuzzy(const float* logits, const int* seq_len, int T, int B, int C, const int* kw,
                                   const int* kw_alt, const int* kw_len, const int* kw_err, int n_kw,
                                   int max_kw_len, float edit_cost, float* score, int* span, int* errors,
                                   int* kw_status, uint32_t* status_word, void* ws, size_t ws_bytes, void* stream) {
    OCRK_REQUIRE(T > 0 && T <= CTC_MAX_T, "ocrk_ctc_spot_fuzzy: T=%d out of range (1..%d)", T, CTC_MAX_T);
    OCRK_REQUIRE(B >= 0 && B <= SPOT_MAX_B && C >= 2 && C <= CTC_MAX_C, "ocrk_ctc_spot_fuzzy: bad B=%d / C=%d", B, C);
    OCRK_REQUIRE(n_kw >= 1 && n_kw <= SPOT_MAX_KW, "ocrk_ctc_spot_fuzzy: n_kw=%d out of range (1..%d)", n_kw,
                 SPOT_MAX_KW);
    OCRK_REQUIRE(max_kw_len >= 1 && max_kw_len <= SPOT_MAX_WIDTH,
                 "ocrk_ctc_spot_fuzzy: max_kw_len=%d out of range (1..%d)", max_kw_len, SPOT_MAX_WIDTH);
    OCRK_REQUIRE(edit_cost >= 0.f, "ocrk_ctc_spot_fuzzy: edit_cost=%g is negative or NaN", (double)edit_cost);
    OCRK_REQUIRE(ws_bytes >= ocrk_ctc_spot_fuzzy_workspace_size(T, B, C, n_kw, max_kw_len),
                 "ocrk_ctc_spot_fuzzy: workspace too small");
    if (B == 0) return OCRK_OK;
    OCRK_REQUIRE(logits && seq_len && kw && kw_len && kw_err && score && span && errors && ws,
                 "ocrk_ctc_spot_fuzzy: null pointer");
    OCRK_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "ocrk_ctc_spot_fuzzy: ws must be 16-B aligned");
    OCRK_REQUIRE((reinterpret_cast<uintptr_t>(span) & 7) == 0, "ocrk_ctc_spot_fuzzy: span must be 8-B aligned");
    hipStream_t s = ocrk::as_stream(stream);
    unsigned char* base = static_cast<unsigned char*>(ws);
    float* tab = reinterpret_cast<float*>(base);
    float2* nba = reinterpret_cast<float2*>(base + fuzzy_tab_bytes(T, B, C));
    int* kinfo = reinterpret_cast<int*>(base + fuzzy_tab_bytes(T, B, C) + fuzzy_nba_bytes(T, B));

    const int frame_blocks = (int)ocrk::cdiv((int64_t)B * T, SPOT_PREP_THREADS / 64);
    const int kw_blocks = (int)ocrk::cdiv(n_kw, SPOT_PREP_THREADS);
    fuzzy_prep_kernel<<<frame_blocks + kw_blocks, SPOT_PREP_THREADS, 0, s>>>(
        logits, seq_len, T, B, C, kw, kw_alt, kw_len, kw_err, n_kw, max_kw_len, tab, nba, kinfo, kw_status,
        status_word, frame_blocks);

    const dim3 grid((unsigned)ocrk::cdiv(n_kw, SPOT_KW), (unsigned)B);
    const int lds_nba = (T * C + 1) & ~1;                  // the pairs are 8-B aligned behind the table
    const size_t dyn = ((size_t)lds_nba + 2 * (size_t)T) * sizeof(float);
    const bool lds = dyn <= SPOT_LDS_MAX && ocrk::opt(ocrk::OPT_CTC_LDS) != 0;   // 0: the table stays in the workspace
    auto launch = lds ? (kw_alt ? fuzzy_launch<true, true> : fuzzy_launch<true, false>)
                      : (kw_alt ? fuzzy_launch<false, true> : fuzzy_launch<false, false>);
    launch(grid, lds ? dyn : 0, s, tab, nba, seq_len, T, C, lds_nba, kw, kw_alt, kw_len, kw_err, kinfo, n_kw,
           max_kw_len, edit_cost, score, span, errors);
    return ocrk::launch_status("ocrk_ctc_spot_fuzzy");
}
