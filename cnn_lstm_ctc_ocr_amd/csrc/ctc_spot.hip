// Keyword spotting on the CTC lattice (ocrk_ctc_spot): for every row of a batch
// and every keyword of a list, the best placement of the keyword INSIDE the row
// -- free start, free end -- as a likelihood ratio against the greedy path, and
// the frames of the hit. The lexicon scorer (ctc_lexicon.hip) answers "which
// word is this whole crop"; this answers "does this line contain TOTAL, where,
// and how much worse than the unconstrained reading is the path that says so".
//
// The score needs no transcendental: with rel[t][c] = logit - max_c logit the
// frame log-sum-exp cancels in the ratio of two paths over the same frames, the
// greedy path scores 0 on every frame, and a Viterbi recursion over
// S = 2 n - 1 states (symbol, blank, symbol, ..., symbol: no leading or
// trailing blank, the frames outside the hit are the greedy filler) is one
// float32 add and three compares per state and frame. include/ocrk.h states
// the recursion and its tie order; tests/ctc_spot_ref.py restates it in NumPy
// and the device is compared with that bit for bit.
//
// (1) spot_prep_kernel: a wave per valid frame writes rel into the workspace
//     table tab[b][t][c]; in further workgroups of the same launch a thread per
//     keyword checks it once (kinfo[k] = the frames it needs, n + the adjacent
//     positions whose label sets overlap, or -1 for a keyword that is not
//     scored; kw_status and the status word's bit are set here). The check
//     happens once per keyword, not once per row, so it needs a launch ahead of
//     the scoring in any case; the table rides in the same launch (measured
//     28.1 us at the serving shape; 29.5 with every scoring workgroup building
//     its LDS table from the raw logits instead).
// (2) spot_score_kernel: grid (chunks of SPOT_KW = 16 keywords) x B, 512 threads.
//     The workgroup copies its row's table into LDS (L C floats), then each of
//     its 8 waves takes a pair of adjacent keywords. State s sits on
//     lane s (R = 1 always: n <= 32, S <= 63); V and the start frame of the
//     path are in registers and move with the whole-wave DPP shifts; the next
//     step's emission is gathered one step ahead. The running best
//     (score, first, end) lives on the lane of state S - 1 and is read out once
//     at the end. Two keywords of at most 16 symbols (S <= 31) share the wave,
//     one per 32-lane half. Nothing is stored per step and there is no barrier
//     after the table copy. When T C floats exceed SPOT_LDS_MAX (or CTC_LDS=0)
//     the waves gather from the workspace table, four steps ahead, with the
//     same expressions in the same order: the same bits.
// No floating-point atomics: a call's outputs are reproducible bit for bit.
#include "ctc_lattice.h"

// Keywords per workgroup and its threads, measured at the serving shape (B = 64, T = 125, C = 96, 64 keywords
// of 3..16 symbols, the C entry, case-sensitive): 16 / 512, a pair per wave, 28.3 us; 8 / 256 29.9; 32 / 1024
// 34.3; 64 / 1024 57.8, 64 / 512 75.9, 64 / 256 151.6 (64 workgroups leave three quarters of the CUs idle: a
// list of keywords is short, so the rows alone do not fill the device). Without pairing 64 / 1024 takes 94.8.
#define SPOT_THREADS 512
#define SPOT_WAVES (SPOT_THREADS / 64)
#define SPOT_KW 16                       // keywords per workgroup: one pair per wave behind one table copy
#define SPOT_MAX_LEN 32                  // S = 2 n - 1 <= 63: one state per lane
#define SPOT_PAIR_LEN 16                 // S <= 31: two such keywords share a wave
#define SPOT_MAX_WIDTH 255               // the label tensor's width (the other CTC entries' limit)
#define SPOT_LDS_MAX (112 * 1024)        // the table's LDS budget (the lexicon scorer's)
#define SPOT_MAX_KW (1 << 20)
#define SPOT_MAX_B 65535                 // rows ride the grid's y dimension
#define SPOT_PREP_THREADS 256

__global__ void __launch_bounds__(SPOT_PREP_THREADS)
spot_prep_kernel(const float* __restrict__ logits, const int* __restrict__ seq_len, int T, int B, int C,
                 const int* __restrict__ kw, const int* __restrict__ kw_alt, const int* __restrict__ kw_len, int n_kw,
                 int max_kw_len, float* __restrict__ tab, int* __restrict__ kinfo, int* __restrict__ kw_status,
                 unsigned* __restrict__ status_word, int frame_blocks) {
    if ((int)blockIdx.x < frame_blocks) {
        ctc_rel_frame<SPOT_PREP_THREADS>(logits, seq_len, T, B, C, tab);
        return;
    }
    // one thread per keyword, with no row in sight. A bad length never indexes the label rows; a bad label
    // or alternative is only ever compared.
    const int k = ((int)blockIdx.x - frame_blocks) * SPOT_PREP_THREADS + threadIdx.x;
    if (k >= n_kw) return;
    const int len = kw_len[k];
    int code = 0, req = -1;
    if (len < 1 || len > SPOT_MAX_LEN || len > max_kw_len) {
        code = 2;
    } else {
        const int* lab = kw + (size_t)k * max_kw_len;
        const int* alt = kw_alt ? kw_alt + (size_t)k * max_kw_len : nullptr;
        bool bad = false;
        int reps = 0, pl = -1, pa = -1;
        for (int i = 0; i < len; ++i) {
            const int l = lab[i], a = alt ? alt[i] : -1;
            bad |= l < 0 || l >= C - 1 || a < -1 || a >= C - 1;
            // positions whose sets {l, a} overlap need the blank between them (pl < 0 at i = 0 matches nothing)
            reps += l == pl || l == pa || (a >= 0 && (a == pl || a == pa));
            pl = l;
            pa = a;
        }
        if (bad) code = 3;
        else req = len + reps;
    }
    kinfo[k] = req;
    if (kw_status) kw_status[k] = code;
    if (code && status_word) __hip_atomic_fetch_or(status_word, 1u << code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// wave_shr1 for an int: lane i takes lane i - 1, lane 0 takes -1
__device__ __forceinline__ int spot_shr1(int v) { return __builtin_amdgcn_update_dpp(-1, v, 0x138, 0xf, 0xf, false); }

// The best placement of one keyword on one wave (PAIR: of two, one per 32-lane
// half; lab, alt and len then differ between the halves, a lane's state is
// lane & 31 and state 0 of the upper half must not take lane 31's value from the
// whole-wave shift; two back is masked by skip already, state 1 never skips).
// tab is the row's [L][C] table of rel (LDS, or the workspace when !LDS); the
// emissions of step t + D are read while step t computes. len is 0 for a
// keyword that is not to be scored here (invalid, needs more than L frames, or
// past the list's end): no lane is active and the result is -inf, (-1, -1).
// The result is returned on every lane of the keyword's half.
template <bool LDS, bool ALT, bool PAIR>
__device__ __forceinline__ void spot_best(const float* __restrict__ tab, const int* __restrict__ lab,
                                          const int* __restrict__ alt, int len, int L, int C, float& score,
                                          int& first, int& end) {
    constexpr int D = LDS ? 1 : 4;                         // one step ahead covers the LDS latency
    const int wlane = threadIdx.x & 63, s = PAIR ? wlane & 31 : wlane, S = 2 * len - 1;
    const bool active = s < S, sym = active && !(s & 1);   // then label index s >> 1 < len
    const int i = s >> 1;
    const int c0 = sym ? lab[i] : C - 1;
    int c1 = c0;                                           // no alternative: the same class twice, max(x, x) = x
    bool skip = false;
    if (sym && i >= 1) {
        const int pl = lab[i - 1];
        skip = c0 != pl;
        if constexpr (ALT) {
            const int a = alt[i], pa = alt[i - 1];
            skip = skip && c0 != pa && (a < 0 || (a != pl && a != pa));
        }
    }
    if constexpr (ALT) {
        if (sym && alt[i] >= 0) c1 = alt[i];
    }
    auto emit = [&](int t) {
        const float e = tab[t * C + c0];
        if constexpr (ALT) return fmaxf(e, tab[t * C + c1]);
        return e;
    };
    float V = -INFINITY, best_v = -INFINITY, en[D];
    int st = -1, best_f = -1, best_e = -1;
#pragma unroll
    for (int d = 0; d < D; ++d) en[d] = emit(min(d, L - 1));
    auto step = [&](float e, int t) {
        float v1 = wave_shr1(V);
        int s1 = spot_shr1(st);
        const float v2 = wave_shr1(v1);
        const int s2 = spot_shr1(s1);
        if constexpr (PAIR) v1 = s == 0 ? -INFINITY : v1;
        float b = V;                                       // stay
        int bs = st;
        if (v1 > b) {                                      // one back, only if strictly greater
            b = v1;
            bs = s1;
        }
        if (skip && v2 > b) {                              // two back, where the two symbol sets are disjoint
            b = v2;
            bs = s2;
        }
        if (s == 0 && 0.f > b) {                           // entry: the filler before the hit scores 0
            b = 0.f;
            bs = t;
        }
        V = active ? b + e : -INFINITY;
        st = bs;
        if (V > best_v) {                                  // read on the lane of state S - 1 only
            best_v = V;
            best_f = st;
            best_e = t + 1;
        }
    };
    // D whole steps per trip, the read ahead clamped to the last frame instead of predicated
    int t0 = 0;
    for (; t0 + D <= L; t0 += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const float e = en[d];
            en[d] = emit(min(t0 + d + D, L - 1));
            step(e, t0 + d);
        }
    }
#pragma unroll
    for (int d = 0; d < D; ++d)
        if (t0 + d < L) step(en[d], t0 + d);
    const int src = (PAIR ? wlane & 32 : 0) + max(S - 1, 0);
    score = __shfl(best_v, src, 64);
    first = __shfl(best_f, src, 64);
    end = __shfl(best_e, src, 64);
}

template <bool LDS, bool ALT>
__global__ void __launch_bounds__(SPOT_THREADS)
spot_score_kernel(const float* __restrict__ tab_g, const int* __restrict__ seq_len, int T, int C,
                  const int* __restrict__ kw, const int* __restrict__ kw_alt, const int* __restrict__ kw_len,
                  const int* __restrict__ kinfo, int n_kw, int max_kw_len, float* __restrict__ score,
                  int* __restrict__ span) {
    extern __shared__ float4 s_dyn4[];                     // LDS: the row's table, [L][C]
    const int b = blockIdx.y;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int L = min(max(seq_len[b], 0), T);
    const int k0 = blockIdx.x * SPOT_KW;
    float* out_v = score + (size_t)b * n_kw;
    int2* out_s = reinterpret_cast<int2*>(span) + (size_t)b * n_kw;
    const float* tab_b = tab_g + (size_t)b * T * C;

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
        }
        return;
    }
    const float* tab = tab_b;
    if constexpr (LDS) {
        const int n = L * C;                               // <= T C floats = the launch's dynamic LDS
        if ((C & 3) == 0) {                                // rows of whole float4s: tab_b is 16-B aligned
            const float4* src = reinterpret_cast<const float4*>(tab_b);
            for (int i = threadIdx.x; i < (n >> 2); i += SPOT_THREADS) s_dyn4[i] = src[i];
        } else {
            float* dst = reinterpret_cast<float*>(s_dyn4);
            for (int i = threadIdx.x; i < n; i += SPOT_THREADS) dst[i] = tab_b[i];
        }
        __syncthreads();
        tab = reinterpret_cast<const float*>(s_dyn4);
    }
    // a wave takes the adjacent keywords 2 p and 2 p + 1 together: both on one pass of the recursion when
    // neither needs more than half a wave, else one after the other
    for (int p = wave; 2 * p < SPOT_KW; p += SPOT_WAVES) {
        int k[2], len[2];                                  // wave-uniform
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            k[h] = k0 + 2 * p + h;
            const int req = k[h] < n_kw ? __builtin_amdgcn_readfirstlane(kinfo[k[h]]) : -1;
            // scored: then the length is in [1, min(32, max_kw_len)]
            len[h] = req >= 0 && req <= L ? __builtin_amdgcn_readfirstlane(kw_len[k[h]]) : 0;
        }
        if (k[0] >= n_kw) break;
        if (len[0] <= SPOT_PAIR_LEN && len[1] <= SPOT_PAIR_LEN) {
            const int h = lane >> 5, kh = h ? k[1] : k[0];
            float v = -INFINITY;
            int f = -1, e = -1;
            if (len[0] | len[1])
                spot_best<LDS, ALT, true>(tab, kw + (size_t)min(kh, n_kw - 1) * max_kw_len,
                                          ALT ? kw_alt + (size_t)min(kh, n_kw - 1) * max_kw_len : nullptr,
                                          h ? len[1] : len[0], L, C, v, f, e);
            if ((lane & 31) == 0 && kh < n_kw) {
                out_v[kh] = v;
                out_s[kh] = make_int2(f, e);
            }
            continue;
        }
#pragma unroll 1
        for (int h = 0; h < 2; ++h) {
            const int kh = h ? k[1] : k[0], n = h ? len[1] : len[0];
            if (kh >= n_kw) break;
            float v = -INFINITY;
            int f = -1, e = -1;
            if (n)
                spot_best<LDS, ALT, false>(tab, kw + (size_t)kh * max_kw_len,
                                           ALT ? kw_alt + (size_t)kh * max_kw_len : nullptr, n, L, C, v, f, e);
            if (lane == 0) {
                out_v[kh] = v;
                out_s[kh] = make_int2(f, e);
            }
        }
    }
}

// ------------------------------------------------------------------- C ABI
static size_t spot_round16(size_t n) { return (n + 15) & ~(size_t)15; }
static bool spot_sizes_ok(int T, int B, int C, int n_kw, int max_kw_len) {
    return T > 0 && T <= CTC_MAX_T && B >= 0 && B <= SPOT_MAX_B && C >= 2 && C <= CTC_MAX_C && n_kw >= 1 &&
           n_kw <= SPOT_MAX_KW && max_kw_len >= 1 && max_kw_len <= SPOT_MAX_WIDTH;
}
static size_t spot_tab_bytes(int T, int B, int C) { return spot_round16((size_t)B * T * C * sizeof(float)); }

extern "C" size_t ocrk_ctc_spot_workspace_size(int T, int B, int C, int n_kw, int max_kw_len) {
    if (!spot_sizes_ok(T, B, C, n_kw, max_kw_len)) return 0;
    return spot_tab_bytes(T, B, C) + spot_round16((size_t)n_kw * sizeof(int));
}

template <bool LDS, bool ALT>
static void spot_launch(dim3 grid, size_t dyn, hipStream_t s, const float* tab, const int* seq_len, int T, int C,
                        const int* kw, const int* kw_alt, const int* kw_len, const int* kinfo, int n_kw,
                        int max_kw_len, float* score, int* span) {
    if constexpr (LDS) {
        static ocrk::DeviceOnce attr;
        ocrk::set_dyn_lds(attr, reinterpret_cast<const void*>(&spot_score_kernel<true, ALT>), SPOT_LDS_MAX);
    }
    spot_score_kernel<LDS, ALT><<<grid, SPOT_THREADS, dyn, s>>>(tab, seq_len, T, C, kw, kw_alt, kw_len, kinfo, n_kw,
                                                               max_kw_len, score, span);
}

extern "C" int ocrk_ctc_spot(const float* logits, const int* seq_len, int T, int B, int C, const int* kw,
                             const int* kw_alt, const int* kw_len, int n_kw, int max_kw_len, float* score, int* span,
                             int* kw_status, uint32_t* status_word, void* ws, size_t ws_bytes, void* stream) {
    OCRK_REQUIRE(T > 0 && T <= CTC_MAX_T, "ocrk_ctc_spot: T=%d out of range (1..%d)", T, CTC_MAX_T);
    OCRK_REQUIRE(B >= 0 && B <= SPOT_MAX_B && C >= 2 && C <= CTC_MAX_C, "ocrk_ctc_spot: bad B=%d / C=%d", B, C);
    OCRK_REQUIRE(n_kw >= 1 && n_kw <= SPOT_MAX_KW, "ocrk_ctc_spot: n_kw=%d out of range (1..%d)", n_kw, SPOT_MAX_KW);
    OCRK_REQUIRE(max_kw_len >= 1 && max_kw_len <= SPOT_MAX_WIDTH, "ocrk_ctc_spot: max_kw_len=%d out of range (1..%d)",
                 max_kw_len, SPOT_MAX_WIDTH);
    OCRK_REQUIRE(ws_bytes >= ocrk_ctc_spot_workspace_size(T, B, C, n_kw, max_kw_len),
                 "ocrk_ctc_spot: workspace too small");
    if (B == 0) return OCRK_OK;
    OCRK_REQUIRE(logits && seq_len && kw && kw_len && score && span && ws, "ocrk_ctc_spot: null pointer");
    OCRK_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "ocrk_ctc_spot: ws must be 16-B aligned");
    OCRK_REQUIRE((reinterpret_cast<uintptr_t>(span) & 7) == 0, "ocrk_ctc_spot: span must be 8-B aligned");
    hipStream_t s = ocrk::as_stream(stream);
    unsigned char* base = static_cast<unsigned char*>(ws);
    float* tab = reinterpret_cast<float*>(base);
    int* kinfo = reinterpret_cast<int*>(base + spot_tab_bytes(T, B, C));

    const int frame_blocks = (int)ocrk::cdiv((int64_t)B * T, SPOT_PREP_THREADS / 64);
    const int kw_blocks = (int)ocrk::cdiv(n_kw, SPOT_PREP_THREADS);
    spot_prep_kernel<<<frame_blocks + kw_blocks, SPOT_PREP_THREADS, 0, s>>>(
        logits, seq_len, T, B, C, kw, kw_alt, kw_len, n_kw, max_kw_len, tab, kinfo, kw_status, status_word,
        frame_blocks);

    const dim3 grid((unsigned)ocrk::cdiv(n_kw, SPOT_KW), (unsigned)B);
    const size_t dyn = (size_t)T * C * sizeof(float);
    const bool lds = dyn <= SPOT_LDS_MAX && ocrk::opt(ocrk::OPT_CTC_LDS) != 0;   // 0: the table stays in the workspace
    auto launch = lds ? (kw_alt ? spot_launch<true, true> : spot_launch<true, false>)
                      : (kw_alt ? spot_launch<false, true> : spot_launch<false, false>);
    launch(grid, lds ? dyn : 0, s, tab, seq_len, T, C, kw, kw_alt, kw_len, kinfo, n_kw, max_kw_len, score, span);
    return ocrk::launch_status("ocrk_ctc_spot");
}
