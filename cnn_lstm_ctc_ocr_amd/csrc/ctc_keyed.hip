// Keyed field reading on the CTC lattice (ocrk_ctc_keyed_field): for every row of a
// batch and every keyed field -- a group of keywords and a pattern -- the jointly
// best placement of one of the keywords, then a gap, then a string matching the
// pattern: "the amount after TOTAL". The spotter (ctc_spot.hip) places a keyword
// and the field reader (ctc_field.hip) places the best matching string anywhere
// in the row; on "TOTAL 12.50 CASH 20.00" a join of their outputs on the host
// cannot recover the amount the field reader did not return, so the join is made
// here, on the lattice, where every placement is still at hand.
//
// include/ocrk.h states the definition; tests/ctc_keyed_ref.py restates it in
// NumPy and the device is compared with that bit for bit. The spotter's and the
// field reader's recursions are not restated: their kernels (ctc_lattice.h) are
// instantiated with a trail written out and an entry value read in.
//
// (1) keyed_prep_kernel: the spotter's frame workgroups write the rel table; in
//     further workgroups of the same launch a thread per keyword and a thread
//     per pattern check them once (kinfo, pinfo, the status outputs); a keyword
//     whose kw_group is outside [0, n_key) is flagged there and never scored.
// (2) spot_score_kernel<.., TRAIL>: the spotter's wave layout; the lane of state
//     S - 1 stores (V, start) of every frame into trail[b][k][t], 8 bytes.
// (3) keyed_gap_kernel: one wave per (row, keyed field) reduces the group's trails
//     into the gap state G[b][a][t] = (value, keyword, keyword first, keyword end):
//     the lanes take 64 frames at a time and find each frame's best keyword (the
//     loads run along t, coalesced), then the carry -- a float32 subtraction per
//     frame, which does not reassociate -- walks the 64 frames through
//     v_readlane, and the lanes store their frames' 16 bytes. No transcendental.
// (4) field_score_kernel<.., KEYED>: the field reader's 16-lane-row layout; the
//     row's G[t] is fetched one frame ahead like the emissions -- on the LDS route
//     from behind the table's row (the table has C + FIELD_PAT floats per frame,
//     so the fetch costs no address register), else from the workspace -- and the
//     epilogue reads G[first] for the keyword outputs.
// No floating-point atomics: a call's outputs are reproducible bit for bit.
#include "ctc_lattice.h"

#define KEYED_PREP_THREADS 256

__global__ void __launch_bounds__(KEYED_PREP_THREADS)
keyed_prep_kernel(const float* __restrict__ logits, const int* __restrict__ seq_len, int T, int B, int C,
                  const int* __restrict__ kw, const int* __restrict__ kw_alt, const int* __restrict__ kw_len,
                  const int* __restrict__ kw_group, int n_kw, int max_kw_len, const int* __restrict__ pat_cls,
                  const int* __restrict__ pat_opt, const int* __restrict__ pat_len, int n_key, int max_pat_len,
                  float* __restrict__ tab, int* __restrict__ kinfo, int* __restrict__ pinfo,
                  int* __restrict__ kw_status, int* __restrict__ pat_status, unsigned* __restrict__ status_word,
                  int frame_blocks, int kw_blocks) {
    if ((int)blockIdx.x < frame_blocks) {
        ctc_rel_frame<KEYED_PREP_THREADS>(logits, seq_len, T, B, C, tab);
        return;
    }
    int code;
    if ((int)blockIdx.x < frame_blocks + kw_blocks) {
        const int k = ((int)blockIdx.x - frame_blocks) * KEYED_PREP_THREADS + threadIdx.x;
        if (k >= n_kw) return;
        int req;
        code = spot_check_keyword(kw, kw_alt, kw_len, k, max_kw_len, C, req);
        const int g = kw_group[k];
        if (!code && (g < 0 || g >= n_key)) {              // belongs to no field: a bad value, never scored
            code = 3;
            req = -1;
        }
        kinfo[k] = req;
        if (kw_status) kw_status[k] = code;
    } else {
        const int p = ((int)blockIdx.x - frame_blocks - kw_blocks) * KEYED_PREP_THREADS + threadIdx.x;
        if (p >= n_key) return;
        int info;
        code = field_check_pattern(pat_cls, pat_opt, pat_len, p, max_pat_len, C, info);
        pinfo[p] = info;
        if (pat_status) pat_status[p] = code;
    }
    if (code && status_word) __hip_atomic_fetch_or(status_word, 1u << code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ float keyed_readlane(float v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// grid n_key x B, one wave. G[0] = (-inf, no keyword); for t >= 1 the candidates are the carry
// G[t - 1].value - gap_cost (only when G[t - 1] has a keyword), then the group's keywords in ascending k with
// trail[k][t - 1], a later one replacing the current only if strictly greater: the first keyword at the
// frame's maximum M, if M is strictly greater than the carry. Only the keywords scored on this row have a
// trail (kinfo in [0, L], as in the trail's kernel).
__global__ void __launch_bounds__(64)
keyed_gap_kernel(const float2* __restrict__ trail, const int* __restrict__ seq_len, int T,
                 const int* __restrict__ kinfo, const int* __restrict__ kw_group, int n_kw, int n_key, float gap_cost,
                 float4* __restrict__ gap) {
    const int a = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    const int L = min(max(seq_len[b], 0), T);
    const float2* trail_b = trail + (size_t)b * n_kw * T;
    float4* out = gap + ((size_t)b * n_key + a) * T;
    float cv = -INFINITY;                                  // the carry, wave-uniform
    int ck = -1, cf = -1, ce = -1;
    for (int t0 = 0; t0 < L; t0 += 64) {
        const int t = t0 + lane;
        float mv = -INFINITY;                              // frame t's best keyword ending exactly at t
        int mk = -1, mf = -1;
        for (int k = 0; k < n_kw; ++k) {                   // wave-uniform trip
            const int req = kinfo[k];
            if (kw_group[k] != a || req < 0 || req > L) continue;
            if (t >= 1 && t < L) {
                const float2 x = trail_b[(size_t)k * T + t - 1];
                if (x.x > mv) {
                    mv = x.x;
                    mk = k;
                    mf = __float_as_int(x.y);
                }
            }
        }
        float4 mine = make_float4(-INFINITY, __int_as_float(-1), __int_as_float(-1), __int_as_float(-1));
        const int n = min(64, L - t0);
        for (int i = 0; i < n; ++i) {
            const float xv = keyed_readlane(mv, i);
            if (ck >= 0) cv = cv - gap_cost;               // one float32 subtraction per frame of gap
            if (xv > cv) {
                cv = xv;
                ck = __builtin_amdgcn_readlane(mk, i);
                cf = __builtin_amdgcn_readlane(mf, i);
                ce = t0 + i;
            }
            if (lane == i) mine = make_float4(cv, __int_as_float(ck), __int_as_float(cf), __int_as_float(ce));
        }
        if (t < L) out[t] = mine;
    }
}

// ------------------------------------------------------------------- C ABI
static size_t keyed_round16(size_t n) { return (n + 15) & ~(size_t)15; }
static bool keyed_sizes_ok(int T, int B, int C, int n_kw, int max_kw_len, int n_key, int max_pat_len) {
    return T > 0 && T <= CTC_MAX_T && B >= 0 && B <= SPOT_MAX_B && C >= 2 && C <= CTC_MAX_C && n_kw >= 1 &&
           n_kw <= SPOT_MAX_KW && max_kw_len >= 1 && max_kw_len <= SPOT_MAX_WIDTH && n_key >= 1 &&
           n_key <= FIELD_MAX_PAT && max_pat_len >= 1 && max_pat_len <= FIELD_MAX_WIDTH;
}
// the workspace: the rel table, a word per keyword, a word per pattern, the trails, the gap states
struct KeyedWs {
    size_t tab, kinfo, pinfo, trail, gap, total;
};
static KeyedWs keyed_ws(int T, int B, int C, int n_kw, int n_key) {
    KeyedWs w;
    w.tab = 0;
    w.kinfo = w.tab + keyed_round16((size_t)B * T * C * sizeof(float));
    w.pinfo = w.kinfo + keyed_round16((size_t)n_kw * sizeof(int));
    w.trail = w.pinfo + keyed_round16((size_t)n_key * sizeof(int));
    w.gap = w.trail + keyed_round16((size_t)B * n_kw * T * sizeof(float2));
    w.total = w.gap + (size_t)B * n_key * T * sizeof(float4);
    return w;
}

extern "C" size_t ocrk_ctc_keyed_field_workspace_size(int T, int B, int C, int n_kw, int max_kw_len, int n_key,
                                                      int max_pat_len) {
    if (!keyed_sizes_ok(T, B, C, n_kw, max_kw_len, n_key, max_pat_len)) return 0;
    return keyed_ws(T, B, C, n_kw, n_key).total;
}

template <bool LDS, bool ALT>
static void keyed_trail_launch(dim3 grid, size_t dyn, hipStream_t s, const float* tab, const int* seq_len, int T,
                               int C, const int* kw, const int* kw_alt, const int* kw_len, const int* kinfo,
                               int n_kw, int max_kw_len, float2* trail) {
    if constexpr (LDS) {
        static ocrk::DeviceOnce attr;
        ocrk::set_dyn_lds(attr, reinterpret_cast<const void*>(&spot_score_kernel<true, ALT, true>), SPOT_LDS_MAX);
    }
    spot_score_kernel<LDS, ALT, true><<<grid, SPOT_THREADS, dyn, s>>>(tab, seq_len, T, C, kw, kw_alt, kw_len, kinfo,
                                                                     n_kw, max_kw_len, nullptr, nullptr, trail);
}

template <bool LDS>
static void keyed_field_launch(dim3 grid, size_t dyn, hipStream_t s, const float* tab, const int* seq_len, int T,
                               int C, const int* pat_cls, const int* pinfo, int n_key, int max_pat_len, float* score,
                               int* span, int* text, const float4* gap, const float2* trail, int n_kw, int* kw_index,
                               float* kw_score) {
    if constexpr (LDS) {
        static ocrk::DeviceOnce attr;
        ocrk::set_dyn_lds(attr, reinterpret_cast<const void*>(&field_score_kernel<true, true>), FIELD_LDS_MAX);
    }
    field_score_kernel<LDS, true><<<grid, FIELD_THREADS, dyn, s>>>(tab, seq_len, T, C, pat_cls, pinfo, n_key,
                                                                  max_pat_len, score, span, text, gap, trail, n_kw,
                                                                  kw_index, kw_score);
}

extern "C" int ocrk_ctc_keyed_field(const float* logits, const int* seq_len, int T, int B, int C, const int* kw,
                                    const int* kw_alt, const int* kw_len, const int* kw_group, int n_kw,
                                    int max_kw_len, const int* pat_cls, const int* pat_opt, const int* pat_len,
                                    int n_key, int max_pat_len, float gap_cost, float* score, int* span, int* kw_index,
                                    float* kw_score, int* text, int* kw_status, int* pat_status,
                                    uint32_t* status_word, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "ocrk_ctc_keyed_field";
    OCRK_REQUIRE(T > 0 && T <= CTC_MAX_T, "%s: T=%d out of range (1..%d)", who, T, CTC_MAX_T);
    OCRK_REQUIRE(B >= 0 && B <= SPOT_MAX_B && C >= 2 && C <= CTC_MAX_C, "%s: bad B=%d / C=%d", who, B, C);
    OCRK_REQUIRE(n_kw >= 1 && n_kw <= SPOT_MAX_KW, "%s: n_kw=%d out of range (1..%d)", who, n_kw, SPOT_MAX_KW);
    OCRK_REQUIRE(max_kw_len >= 1 && max_kw_len <= SPOT_MAX_WIDTH, "%s: max_kw_len=%d out of range (1..%d)", who,
                 max_kw_len, SPOT_MAX_WIDTH);
    OCRK_REQUIRE(n_key >= 1 && n_key <= FIELD_MAX_PAT, "%s: n_key=%d out of range (1..%d)", who, n_key, FIELD_MAX_PAT);
    OCRK_REQUIRE(max_pat_len >= 1 && max_pat_len <= FIELD_MAX_WIDTH, "%s: max_pat_len=%d out of range (1..%d)", who,
                 max_pat_len, FIELD_MAX_WIDTH);
    OCRK_REQUIRE(gap_cost >= 0.f, "%s: gap_cost=%g is negative or NaN", who, (double)gap_cost);
    OCRK_REQUIRE(ws_bytes >= ocrk_ctc_keyed_field_workspace_size(T, B, C, n_kw, max_kw_len, n_key, max_pat_len),
                 "%s: workspace too small", who);
    if (B == 0) return OCRK_OK;
    OCRK_REQUIRE(logits && seq_len && kw && kw_len && kw_group && pat_cls && pat_opt && pat_len && score && span &&
                     kw_index && kw_score && text && ws,
                 "%s: null pointer", who);
    OCRK_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "%s: ws must be 16-B aligned", who);
    OCRK_REQUIRE((reinterpret_cast<uintptr_t>(span) & 15) == 0, "%s: span must be 16-B aligned", who);
    hipStream_t s = ocrk::as_stream(stream);
    unsigned char* base = static_cast<unsigned char*>(ws);
    const KeyedWs w = keyed_ws(T, B, C, n_kw, n_key);
    float* tab = reinterpret_cast<float*>(base + w.tab);
    int* kinfo = reinterpret_cast<int*>(base + w.kinfo);
    int* pinfo = reinterpret_cast<int*>(base + w.pinfo);
    float2* trail = reinterpret_cast<float2*>(base + w.trail);
    float4* gap = reinterpret_cast<float4*>(base + w.gap);

    const int frame_blocks = (int)ocrk::cdiv((int64_t)B * T, KEYED_PREP_THREADS / 64);
    const int kw_blocks = (int)ocrk::cdiv(n_kw, KEYED_PREP_THREADS);
    const int pat_blocks = (int)ocrk::cdiv(n_key, KEYED_PREP_THREADS);
    keyed_prep_kernel<<<frame_blocks + kw_blocks + pat_blocks, KEYED_PREP_THREADS, 0, s>>>(
        logits, seq_len, T, B, C, kw, kw_alt, kw_len, kw_group, n_kw, max_kw_len, pat_cls, pat_opt, pat_len, n_key,
        max_pat_len, tab, kinfo, pinfo, kw_status, pat_status, status_word, frame_blocks, kw_blocks);

    const bool want_lds = ocrk::opt(ocrk::OPT_CTC_LDS) != 0;   // 0: the table stays in the workspace
    {
        const size_t dyn = (size_t)T * C * sizeof(float);
        const bool lds = dyn <= SPOT_LDS_MAX && want_lds;
        const dim3 grid((unsigned)ocrk::cdiv(n_kw, SPOT_KW), (unsigned)B);
        auto launch = lds ? (kw_alt ? keyed_trail_launch<true, true> : keyed_trail_launch<true, false>)
                          : (kw_alt ? keyed_trail_launch<false, true> : keyed_trail_launch<false, false>);
        launch(grid, lds ? dyn : 0, s, tab, seq_len, T, C, kw, kw_alt, kw_len, kinfo, n_kw, max_kw_len, trail);
    }
    keyed_gap_kernel<<<dim3((unsigned)n_key, (unsigned)B), 64, 0, s>>>(trail, seq_len, T, kinfo, kw_group, n_kw, n_key,
                                                                       gap_cost, gap);
    {
        const size_t dyn = (size_t)T * (C + FIELD_PAT) * sizeof(float);   // the table and the entry values behind it
        const bool lds = dyn <= FIELD_LDS_MAX && want_lds;
        const dim3 grid((unsigned)ocrk::cdiv(n_key, FIELD_PAT), (unsigned)B);
        auto launch = lds ? keyed_field_launch<true> : keyed_field_launch<false>;
        launch(grid, lds ? dyn : 0, s, tab, seq_len, T, C, pat_cls, pinfo, n_key, max_pat_len, score, span, text, gap,
               trail, n_kw, kw_index, kw_score);
    }
    return ocrk::launch_status("ocrk_ctc_keyed_field");
}
