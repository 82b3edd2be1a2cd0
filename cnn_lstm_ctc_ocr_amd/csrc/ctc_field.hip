// Field reading on the CTC lattice (ocrk_ctc_field): for every row of a batch
// and every pattern of a list, the best-scoring string that matches the pattern
// -- a sequence of up to 16 character classes, some optional -- placed anywhere
// inside the row, as a likelihood ratio against the greedy path, with the frames
// of the hit and the label chosen at each position. The keyword spotter
// (ctc_spot.hip) finds "TOTAL"; this reads the amount next to it without
// enumerating the million strings [1-9]\d{0,3}\.\d{1,2} matches.
//
// The score is the spotter's: rel[t][c] = logit - max_c logit, the greedy path
// scores 0 on every frame, one float32 add per state and frame, no
// transcendental. include/ocrk.h states the recursion and its tie order;
// tests/ctc_field_ref.py restates it in NumPy and the device is compared with
// that bit for bit.
//
// (1) field_prep_kernel: the spotter's frame workgroups (ctc_lattice.h) write
//     the rel table; in further workgroups of the same launch a thread per
//     pattern checks it once (pinfo[p] = its length and optional flags, or -1
//     for a pattern that is not scored; pat_status and the status word's bit
//     are set here).
// (2) field_score_kernel: grid (chunks of FIELD_PAT = 8 patterns) x B, 128
//     threads. The workgroup copies its row's table into LDS, then every
//     16-lane DPP row of its two waves takes one pattern: lane j holds the
//     state "position i emits the class's j-th label" of EVERY position, the
//     positions unrolled in registers (templated on 4 / 8 / 16 of them, the
//     pattern right-aligned so that the end positions are compile-time
//     registers), and a copy of the row-uniform blank states. A position's
//     top-2 over its 17 states -- all a successor needs, since at most one
//     state carries the successor's own label -- is two maxima by row
//     rotations, each followed by a ballot for its first lane; the path's start frame and chosen labels
//     (a nibble per position, a presence mask) ride in three registers and are
//     fetched from the winning lanes by ds_bpermute. Nothing is stored per frame
//     and there is no barrier after the table copy. When T C floats exceed
//     FIELD_LDS_MAX (or CTC_LDS=0) the rows gather from the workspace table with
//     the same expressions in the same order: the same bits.
// No floating-point atomics: a call's outputs are reproducible bit for bit.
#include "ctc_lattice.h"

__global__ void __launch_bounds__(FIELD_PREP_THREADS)
field_prep_kernel(const float* __restrict__ logits, const int* __restrict__ seq_len, int T, int B, int C,
                  const int* __restrict__ pat_cls, const int* __restrict__ pat_opt, const int* __restrict__ pat_len,
                  int n_pat, int max_pat_len, float* __restrict__ tab, int* __restrict__ pinfo,
                  int* __restrict__ pat_status, unsigned* __restrict__ status_word, int frame_blocks) {
    if ((int)blockIdx.x < frame_blocks) {
        ctc_rel_frame<FIELD_PREP_THREADS>(logits, seq_len, T, B, C, tab);
        return;
    }
    // one thread per pattern, with no row in sight (field_check_pattern, ctc_lattice.h)
    const int p = ((int)blockIdx.x - frame_blocks) * FIELD_PREP_THREADS + threadIdx.x;
    if (p >= n_pat) return;
    int info;
    const int code = field_check_pattern(pat_cls, pat_opt, pat_len, p, max_pat_len, C, info);
    pinfo[p] = info;
    if (pat_status) pat_status[p] = code;
    if (code && status_word) __hip_atomic_fetch_or(status_word, 1u << code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ------------------------------------------------------------------- C ABI
static size_t field_round16(size_t n) { return (n + 15) & ~(size_t)15; }
static bool field_sizes_ok(int T, int B, int C, int n_pat, int max_pat_len) {
    return T > 0 && T <= CTC_MAX_T && B >= 0 && B <= FIELD_MAX_B && C >= 2 && C <= CTC_MAX_C && n_pat >= 1 &&
           n_pat <= FIELD_MAX_PAT && max_pat_len >= 1 && max_pat_len <= FIELD_MAX_WIDTH;
}
static size_t field_tab_bytes(int T, int B, int C) { return field_round16((size_t)B * T * C * sizeof(float)); }

extern "C" size_t ocrk_ctc_field_workspace_size(int T, int B, int C, int n_pat, int max_pat_len) {
    if (!field_sizes_ok(T, B, C, n_pat, max_pat_len)) return 0;
    return field_tab_bytes(T, B, C) + field_round16((size_t)n_pat * sizeof(int));
}

template <bool LDS>
static void field_launch(dim3 grid, size_t dyn, hipStream_t s, const float* tab, const int* seq_len, int T, int C,
                         const int* pat_cls, const int* pinfo, int n_pat, int max_pat_len, float* score, int* span,
                         int* text) {
    if constexpr (LDS) {
        static ocrk::DeviceOnce attr;
        ocrk::set_dyn_lds(attr, reinterpret_cast<const void*>(&field_score_kernel<true, false>), FIELD_LDS_MAX);
    }
    field_score_kernel<LDS, false><<<grid, FIELD_THREADS, dyn, s>>>(tab, seq_len, T, C, pat_cls, pinfo, n_pat,
                                                                   max_pat_len, score, span, text, nullptr, nullptr, 0,
                                                                   nullptr, nullptr);
}

extern "C" int ocrk_ctc_field(const float* logits, const int* seq_len, int T, int B, int C, const int* pat_cls,
                              const int* pat_opt, const int* pat_len, int n_pat, int max_pat_len, float* score,
                              int* span, int* text, int* pat_status, uint32_t* status_word, void* ws, size_t ws_bytes,
                              void* stream) {
    OCRK_REQUIRE(T > 0 && T <= CTC_MAX_T, "ocrk_ctc_field: T=%d out of range (1..%d)", T, CTC_MAX_T);
    OCRK_REQUIRE(B >= 0 && B <= FIELD_MAX_B && C >= 2 && C <= CTC_MAX_C, "ocrk_ctc_field: bad B=%d / C=%d", B, C);
    OCRK_REQUIRE(n_pat >= 1 && n_pat <= FIELD_MAX_PAT, "ocrk_ctc_field: n_pat=%d out of range (1..%d)", n_pat,
                 FIELD_MAX_PAT);
    OCRK_REQUIRE(max_pat_len >= 1 && max_pat_len <= FIELD_MAX_WIDTH,
                 "ocrk_ctc_field: max_pat_len=%d out of range (1..%d)", max_pat_len, FIELD_MAX_WIDTH);
    OCRK_REQUIRE(ws_bytes >= ocrk_ctc_field_workspace_size(T, B, C, n_pat, max_pat_len),
                 "ocrk_ctc_field: workspace too small");
    if (B == 0) return OCRK_OK;
    OCRK_REQUIRE(logits && seq_len && pat_cls && pat_opt && pat_len && score && span && text && ws,
                 "ocrk_ctc_field: null pointer");
    OCRK_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "ocrk_ctc_field: ws must be 16-B aligned");
    OCRK_REQUIRE((reinterpret_cast<uintptr_t>(span) & 7) == 0, "ocrk_ctc_field: span must be 8-B aligned");
    hipStream_t s = ocrk::as_stream(stream);
    unsigned char* base = static_cast<unsigned char*>(ws);
    float* tab = reinterpret_cast<float*>(base);
    int* pinfo = reinterpret_cast<int*>(base + field_tab_bytes(T, B, C));

    const int frame_blocks = (int)ocrk::cdiv((int64_t)B * T, FIELD_PREP_THREADS / 64);
    const int pat_blocks = (int)ocrk::cdiv(n_pat, FIELD_PREP_THREADS);
    field_prep_kernel<<<frame_blocks + pat_blocks, FIELD_PREP_THREADS, 0, s>>>(
        logits, seq_len, T, B, C, pat_cls, pat_opt, pat_len, n_pat, max_pat_len, tab, pinfo, pat_status, status_word,
        frame_blocks);

    const dim3 grid((unsigned)ocrk::cdiv(n_pat, FIELD_PAT), (unsigned)B);
    const size_t dyn = (size_t)T * C * sizeof(float);
    const bool lds = dyn <= FIELD_LDS_MAX && ocrk::opt(ocrk::OPT_CTC_LDS) != 0;   // 0: the table stays in the workspace
    auto launch = lds ? field_launch<true> : field_launch<false>;
    launch(grid, lds ? dyn : 0, s, tab, seq_len, T, C, pat_cls, pinfo, n_pat, max_pat_len, score, span, text);
    return ocrk::launch_status("ocrk_ctc_field");
}
