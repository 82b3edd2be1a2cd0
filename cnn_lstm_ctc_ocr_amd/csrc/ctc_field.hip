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

#define FIELD_THREADS 128
#define FIELD_PAT (FIELD_THREADS / 16)    // patterns per workgroup: one per 16-lane row behind one table copy
#define FIELD_MAX_LEN 16                  // positions: a 4-bit class index each in two registers
#define FIELD_CLASS 16                    // labels per class: one per lane of a DPP row
#define FIELD_MAX_OPT 3                   // consecutive optional positions: at most 4 predecessors
#define FIELD_MAX_WIDTH 255               // the pattern tensors' width (the other CTC entries' limit)
#define FIELD_LDS_MAX (112 * 1024)        // the table's LDS budget (the spotter's and the lexicon scorer's)
#define FIELD_MAX_PAT (1 << 20)
#define FIELD_MAX_B 65535                 // rows ride the grid's y dimension
#define FIELD_PREP_THREADS 256

__global__ void __launch_bounds__(FIELD_PREP_THREADS)
field_prep_kernel(const float* __restrict__ logits, const int* __restrict__ seq_len, int T, int B, int C,
                  const int* __restrict__ pat_cls, const int* __restrict__ pat_opt, const int* __restrict__ pat_len,
                  int n_pat, int max_pat_len, float* __restrict__ tab, int* __restrict__ pinfo,
                  int* __restrict__ pat_status, unsigned* __restrict__ status_word, int frame_blocks) {
    if ((int)blockIdx.x < frame_blocks) {
        ctc_rel_frame<FIELD_PREP_THREADS>(logits, seq_len, T, B, C, tab);
        return;
    }
    // one thread per pattern, with no row in sight. A bad length never indexes the pattern's rows; a label is
    // only ever compared.
    const int p = ((int)blockIdx.x - frame_blocks) * FIELD_PREP_THREADS + threadIdx.x;
    if (p >= n_pat) return;
    const int len = pat_len[p];
    int code = 0, info = -1;
    if (len < 1 || len > FIELD_MAX_LEN || len > max_pat_len) {
        code = 2;
    } else {
        const int* opt = pat_opt + (size_t)p * max_pat_len;
        const int* cls = pat_cls + (size_t)p * max_pat_len * FIELD_CLASS;
        bool bad_structure = opt[0] != 0, bad_label = false;
        int run = 0, mask = 0;
        for (int i = 0; i < len; ++i) {
            const bool o = opt[i] != 0;
            run = o ? run + 1 : 0;
            bad_structure |= run > FIELD_MAX_OPT;
            mask |= (int)o << i;
            int prev = -1;
            bool ended = false;
            for (int j = 0; j < FIELD_CLASS; ++j) {          // 1..16 labels strictly ascending, then -1s
                const int l = cls[i * FIELD_CLASS + j];
                if (l == -1) {
                    ended = true;
                    bad_label |= j == 0;
                    continue;
                }
                bad_label |= ended || l < 0 || l >= C - 1 || l <= prev;
                prev = l;
            }
        }
        code = bad_structure ? 2 : bad_label ? 3 : 0;
        if (!code) info = len | (mask << 8);
    }
    pinfo[p] = info;
    if (pat_status) pat_status[p] = code;
    if (code && status_word) __hip_atomic_fetch_or(status_word, 1u << code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The maximum over a 16-lane DPP row by rotations: every lane gets the row's result. The rotation rides in the
// v_max_f32 itself (for fmaxf(v, dpp(v)) the compiler keeps a v_mov_b32_dpp, a wait and a canonicalising second
// v_max_f32 per step: four instructions where this has two); a DPP operand written by the VALU instruction
// before it needs two wait states. No NaN is ever an operand (V is a sum of rel values, or -inf).
__device__ __forceinline__ float field_row_max(float v) {
    float r;
    asm("s_nop 1\n\t"
        "v_max_f32_dpp %0, %1, %1 row_ror:8 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_max_f32_dpp %0, %0, %0 row_ror:4 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_max_f32_dpp %0, %0, %0 row_ror:2 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_max_f32_dpp %0, %0, %0 row_ror:1 row_mask:0xf bank_mask:0xf"
        : "=v"(r)
        : "v"(v));
    return r;
}
// The lowest / highest lane (0..15) of this lane's row on which c holds, from the wave's ballot: a compare, a
// shift and a bit scan where a min / max reduction of lane indices takes four rotations. `none` if there is
// no such lane.
__device__ __forceinline__ unsigned field_row_bits(bool c, int row0) {
    return (unsigned)(__builtin_amdgcn_ballot_w64(c) >> row0) & 0xffffu;
}
__device__ __forceinline__ int field_row_first(bool c, int row0, int none) {
    const unsigned bits = field_row_bits(c, row0);
    return bits ? __builtin_ctz(bits) : none;
}
__device__ __forceinline__ int field_row_last(bool c, int row0, int none) {
    const unsigned bits = field_row_bits(c, row0);
    return bits ? 31 - __builtin_clz(bits) : none;
}

// What a state carries besides V: the class index chosen at registers 0..7 (a) and 8..15 (b, only N > 8), a
// nibble each; the frame at which the path entered position 0 (m >> 16) and the registers present (m & 0xffff).
template <int N>
struct FieldPay {
    unsigned a, b, m;
};
template <int N>
__device__ __forceinline__ FieldPay<N> field_sel(bool c, const FieldPay<N>& x, const FieldPay<N>& y) {
    FieldPay<N> r;
    r.a = c ? x.a : y.a;
    r.b = 0;
    if constexpr (N > 8) r.b = c ? x.b : y.b;
    r.m = c ? x.m : y.m;
    return r;
}
// every lane reads lane `src` (an index within the wave); all lanes of the wave take part
template <int N>
__device__ __forceinline__ FieldPay<N> field_from(const FieldPay<N>& x, int src) {
    FieldPay<N> r;
    r.a = (unsigned)__builtin_amdgcn_ds_bpermute(src << 2, (int)x.a);
    r.b = 0;
    if constexpr (N > 8) r.b = (unsigned)__builtin_amdgcn_ds_bpermute(src << 2, (int)x.b);
    r.m = (unsigned)__builtin_amdgcn_ds_bpermute(src << 2, (int)x.m);
    return r;
}

// The best match of one pattern per 16-lane row (four rows per wave, each with its own pattern; `info` is
// pinfo's word, 0 for a row with nothing to score: every state of such a row stays at -inf). The pattern's
// position i sits in register i + N - len, so the end positions are registers N - 1 .. N - 4 whatever the
// length; lane j of the row holds the state of the class's j-th label of every register. tab is the row's
// [L][C] table of rel (LDS or the workspace); the emissions of frame t + 1 are read while frame t computes.
// nmax is the longest pattern of the wave (wave-uniform): the registers below N - nmax hold nothing on any row
// and are skipped.
// Returns the score and span on every lane of the row, and on lane i the label chosen at position i (-1 for
// an absent position, for i >= len, and when nothing matched).
template <int N>
__device__ __forceinline__ void field_best(const float* __restrict__ tab, const int* __restrict__ cls, int info,
                                           int nmax, int L, int C, float& score, int& first, int& end, int& label) {
    using Pay = FieldPay<N>;
    const int lane16 = threadIdx.x & 15, row0 = threadIdx.x & 48;
    const int len = info & 255, shift = N - len;
    const unsigned optr = (unsigned)(info >> 8) << shift;    // bit r: register r's position is optional
    // bit r of allow[d]: register r may be entered from register r - d - 1 (everything between is optional)
    unsigned allow[FIELD_MAX_OPT];
    allow[0] = optr << 1;
    allow[1] = allow[0] & (optr << 2);
    allow[2] = allow[1] & (optr << 3);
    // wave-uniform bounds, so that a wave of short-cut-free patterns skips the far predecessors and ends
    const int dmax = 1 + (__builtin_amdgcn_ballot_w64(allow[0] != 0) != 0) +
                     (__builtin_amdgcn_ballot_w64(allow[1] != 0) != 0) +
                     (__builtin_amdgcn_ballot_w64(allow[2] != 0) != 0);
    // end register N - 1 - d counts if the d registers after it are optional
    bool endok[FIELD_MAX_OPT + 1];
    endok[0] = len > 0;
#pragma unroll
    for (int d = 1; d <= FIELD_MAX_OPT; ++d) endok[d] = endok[d - 1] && ((optr >> (N - d)) & 1u);
    const int emax = 1 + (__builtin_amdgcn_ballot_w64(endok[1]) != 0) + (__builtin_amdgcn_ballot_w64(endok[2]) != 0) +
                     (__builtin_amdgcn_ballot_w64(endok[3]) != 0);

    int lab[N];                                              // this lane's label at each register, -1 for none
#pragma unroll
    for (int r = 0; r < N; ++r) lab[r] = r >= shift && len > 0 ? cls[(r - shift) * FIELD_CLASS + lane16] : -1;

    float Vs[N], Vb[N], en[N], enb;
    Pay Ps[N], Pb[N];
#pragma unroll
    for (int r = 0; r < N; ++r) {
        Vs[r] = Vb[r] = en[r] = -INFINITY;
        Ps[r] = Pb[r] = Pay{0u, 0u, 0u};
    }
    auto gather = [&](int t) {
        const float* row = tab + t * C;
#pragma unroll
        for (int r = 0; r < N; ++r) {
            if (r < N - nmax) continue;
            const float e = row[max(lab[r], 0)];
            en[r] = lab[r] >= 0 ? e : -INFINITY;
        }
        enb = row[C - 1];
    };
    float best_v = -INFINITY;
    int best_s = -1, best_e = -1;
    Pay best_p{0u, 0u, 0u};
    gather(0);
    for (int t = 0; t < L; ++t) {
        float e[N];
#pragma unroll
        for (int r = 0; r < N; ++r) e[r] = en[r];
        const float eb = enb;
        gather(min(t + 1, L - 1));
        // the top-2 of each register's 17 states of frame t - 1 (blank first, then the labels ascending; the
        // lowest on ties), with what they carry; only the last four stay live
        float t1v[N], t2v[N];
        int t1l[N];
        Pay t1p[N], t2p[N];
#pragma unroll
        for (int r = 0; r < N; ++r) {
            if (r < N - nmax) {                              // no row of the wave uses the register: never a source
                t1v[r] = t2v[r] = -INFINITY;
                t1l[r] = -1;
                t1p[r] = t2p[r] = Pay{0u, 0u, 0u};
                continue;
            }
            const float v = Vs[r];
            // the labels ascend with the lane: the lowest lane at the maximum is the first in the order
            const float m1 = field_row_max(v);
            const int j1 = field_row_first(v == m1, row0, 0);
            const float x = lane16 == j1 ? -INFINITY : v;
            const float m2 = field_row_max(x);
            const int j2 = field_row_first(x == m2 && lane16 != j1, row0, 0);
            const Pay p1 = field_from<N>(Ps[r], row0 + j1);
            const Pay p2 = field_from<N>(Ps[r], row0 + j2);
            const int l1 = __builtin_amdgcn_ds_bpermute((row0 + j1) << 2, lab[r]);
            const float vb = Vb[r];
            const bool bf = vb >= m1, bs = vb >= m2;         // the blank comes first among equals
            t1v[r] = bf ? vb : m1;
            t1l[r] = bf ? -1 : l1;
            t1p[r] = field_sel<N>(bf, Pb[r], p1);
            t2v[r] = bf ? m1 : (bs ? vb : m2);
            t2p[r] = field_sel<N>(bf, p1, field_sel<N>(bs, Pb[r], p2));
            // the blank after the position: itself, then the position's labels
            Vb[r] = t1v[r] + eb;
            Pb[r] = t1p[r];
            // the label: stay, then the predecessors nearest first, each without the state of the same label
            float b = v;
            Pay p = Ps[r];
#pragma unroll
            for (int d = 1; d <= FIELD_MAX_OPT + 1; ++d) {
                if (r - d < 0 || d > dmax) continue;
                const bool same = t1l[r - d] == lab[r];
                const float cv = same ? t2v[r - d] : t1v[r - d];
                const bool take = cv > b && (d == 1 || ((allow[d > 1 ? d - 2 : 0] >> r) & 1u));
                b = take ? cv : b;
                p = field_sel<N>(take, field_sel<N>(same, t2p[r - d], t1p[r - d]), p);
            }
            if (r == shift && 0.f > b) {                     // the free start: the filler before the hit scores 0
                b = 0.f;
                p = Pay{0u, 0u, (unsigned)t << 16};
            }
            Vs[r] = b + e[r];
            if (r < 8) p.a |= (unsigned)lane16 << (4 * (r & 7));
            else p.b |= (unsigned)lane16 << (4 * (r & 7));
            p.m |= 1u << r;
            Ps[r] = p;
        }
        // the row's best: the end registers nearest to N - 1 first, the labels ascending within each. In that
        // order a candidate replaces the best if it is strictly greater, or equal (finite) with the same start;
        // within one register that is: the LAST lane at the register's maximum M whose start is that of the
        // FIRST lane at M (M greater than the best) or the best's (M equal to it).
#pragma unroll
        for (int d = 0; d <= FIELD_MAX_OPT; ++d) {
            if (d >= N || d >= emax) continue;
            const int r = N - 1 - d;
            const float v = Vs[r];
            const float M = field_row_max(v);
            const bool bigger = M > best_v, equal = M == best_v && best_v > -INFINITY;
            const int jf = field_row_first(v == M, row0, 0);
            const int st = (int)(Ps[r].m >> 16);
            const int sf = __builtin_amdgcn_ds_bpermute((row0 + jf) << 2, st);
            const int sref = bigger ? sf : best_s;
            const int jl = field_row_last(v == M && st == sref, row0, -1);
            const Pay pl = field_from<N>(Ps[r], row0 + max(jl, 0));
            const bool take = endok[d] && (bigger || equal) && jl >= 0;
            best_v = take ? M : best_v;
            best_s = take ? sref : best_s;
            best_e = take ? t + 1 : best_e;
            best_p = field_sel<N>(take, pl, best_p);
        }
    }
    score = best_v;
    first = best_s;
    end = best_e;
    // lane i reports position i = register i + shift
    const int r = lane16 + shift;
    label = -1;
    if (lane16 < len && best_e >= 0 && ((best_p.m >> r) & 1u)) {
        const unsigned word = r < 8 ? best_p.a : best_p.b;
        label = cls[lane16 * FIELD_CLASS + (int)((word >> (4 * (r & 7))) & 15u)];
    }
}

template <bool LDS>
__global__ void __launch_bounds__(FIELD_THREADS)
field_score_kernel(const float* __restrict__ tab_g, const int* __restrict__ seq_len, int T, int C,
                   const int* __restrict__ pat_cls, const int* __restrict__ pinfo, int n_pat, int max_pat_len,
                   float* __restrict__ score, int* __restrict__ span, int* __restrict__ text) {
    extern __shared__ float4 s_dyn4[];                     // LDS: the row's table, [L][C]
    const int b = blockIdx.y;
    const int lane16 = threadIdx.x & 15;
    const int L = min(max(seq_len[b], 0), T);
    const int p = blockIdx.x * FIELD_PAT + ((int)threadIdx.x >> 4);
    const float* tab_b = tab_g + (size_t)b * T * C;

    int info = 0;                                          // 0: nothing to score on this DPP row
    if (p < n_pat && L > 0) info = max(pinfo[p], 0);       // a valid pattern: its length (>= 1) and optional flags
    float v = -INFINITY;
    int f = -1, e = -1, label = -1;
    if (__syncthreads_or(info != 0)) {
        const float* tab = tab_b;
        if constexpr (LDS) {
            const int n = L * C;                           // <= T C floats = the launch's dynamic LDS
            if ((C & 3) == 0) {                            // rows of whole float4s: tab_b is 16-B aligned
                const float4* src = reinterpret_cast<const float4*>(tab_b);
                for (int i = threadIdx.x; i < (n >> 2); i += FIELD_THREADS) s_dyn4[i] = src[i];
            } else {
                float* dst = reinterpret_cast<float*>(s_dyn4);
                for (int i = threadIdx.x; i < n; i += FIELD_THREADS) dst[i] = tab_b[i];
            }
            __syncthreads();
            tab = reinterpret_cast<const float*>(s_dyn4);
        }
        // the wave's longest pattern picks the unrolling
        const int len = info & 255;
        const int nmax = max(max(__builtin_amdgcn_readlane(len, 0), __builtin_amdgcn_readlane(len, 16)),
                             max(__builtin_amdgcn_readlane(len, 32), __builtin_amdgcn_readlane(len, 48)));
        const int* cls = pat_cls + (size_t)min(p, n_pat - 1) * max_pat_len * FIELD_CLASS;
        if (nmax > 8) field_best<16>(tab, cls, info, nmax, L, C, v, f, e, label);
        else if (nmax > 4) field_best<8>(tab, cls, info, nmax, L, C, v, f, e, label);
        else if (nmax > 0) field_best<4>(tab, cls, info, nmax, L, C, v, f, e, label);
    }
    if (p >= n_pat) return;
    const size_t o = (size_t)b * n_pat + p;
    if (lane16 == 0) {
        score[o] = v;
        reinterpret_cast<int2*>(span)[o] = make_int2(f, e);
    }
    for (int i = lane16; i < max_pat_len; i += 16) text[o * max_pat_len + i] = i < FIELD_MAX_LEN ? label : -1;
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
        ocrk::set_dyn_lds(attr, reinterpret_cast<const void*>(&field_score_kernel<true>), FIELD_LDS_MAX);
    }
    field_score_kernel<LDS><<<grid, FIELD_THREADS, dyn, s>>>(tab, seq_len, T, C, pat_cls, pinfo, n_pat, max_pat_len,
                                                            score, span, text);
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
