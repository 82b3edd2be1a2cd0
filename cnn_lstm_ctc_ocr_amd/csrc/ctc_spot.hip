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
// SPOT_KW, SPOT_THREADS and the kernel itself are in ctc_lattice.h: the keyed field reader runs it too.

__global__ void __launch_bounds__(SPOT_PREP_THREADS)
spot_prep_kernel(const float* __restrict__ logits, const int* __restrict__ seq_len, int T, int B, int C,
                 const int* __restrict__ kw, const int* __restrict__ kw_alt, const int* __restrict__ kw_len, int n_kw,
                 int max_kw_len, float* __restrict__ tab, int* __restrict__ kinfo, int* __restrict__ kw_status,
                 unsigned* __restrict__ status_word, int frame_blocks) {
    if ((int)blockIdx.x < frame_blocks) {
        ctc_rel_frame<SPOT_PREP_THREADS>(logits, seq_len, T, B, C, tab);
        return;
    }
    // one thread per keyword, with no row in sight (spot_check_keyword, ctc_lattice.h)
    const int k = ((int)blockIdx.x - frame_blocks) * SPOT_PREP_THREADS + threadIdx.x;
    if (k >= n_kw) return;
    int req;
    const int code = spot_check_keyword(kw, kw_alt, kw_len, k, max_kw_len, C, req);
    kinfo[k] = req;
    if (kw_status) kw_status[k] = code;
    if (code && status_word) __hip_atomic_fetch_or(status_word, 1u << code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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
        ocrk::set_dyn_lds(attr, reinterpret_cast<const void*>(&spot_score_kernel<true, ALT, false>), SPOT_LDS_MAX);
    }
    spot_score_kernel<LDS, ALT, false><<<grid, SPOT_THREADS, dyn, s>>>(tab, seq_len, T, C, kw, kw_alt, kw_len, kinfo,
                                                                      n_kw, max_kw_len, score, span, nullptr);
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
