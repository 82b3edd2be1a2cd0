// The extended-label lattice helpers shared by the CTC loss / alignment
// (ctc.hip) and the lexicon scorer (ctc_lexicon.hip): base-2 log-sum-exps and
// the state shifts of a lattice held in the registers of one wave (lane j
// holds states j, j + 64, ...: R registers); the rel table of the keyword
// spotter (ctc_spot.hip) and the field reader (ctc_field.hip); and those two
// entries' checks, recursions and score kernels, which the keyed field reader
// (ctc_keyed.hip) instantiates with a trail written out and an entry value
// read in.
#pragma once
#include <cfloat>

#include "common.h"

#define CTC_MAX_R 8                 // S <= 512  (labels up to 255 symbols)
#define CTC_MAX_T 4096
#define CTC_MAX_C 256

// The lattices and emissions hold log2 probabilities: the log-sum-exps are
// then v_exp_f32 / v_log_f32 (base-2 hardware transcendentals, one
// instruction each) instead of the libm expf / logf sequences, on the
// recursion's serial chain. The -FLT_MAX floor keeps an all -inf argument
// list NaN-free without a branch (2^-inf = 0, log2 0 = -inf).
constexpr float LOG2E_F = 1.4426950408889634f, LN2_F = 0.6931471805599453f;
__device__ __forceinline__ float lse2b(float a, float b) {
    const float m = fmaxf(fmaxf(a, b), -FLT_MAX);
    return m + __builtin_amdgcn_logf(__builtin_amdgcn_exp2f(a - m) + __builtin_amdgcn_exp2f(b - m));
}
__device__ __forceinline__ float lse3b(float a, float b, float c) {
    const float m = fmaxf(fmaxf(fmaxf(a, b), c), -FLT_MAX);
    return m + __builtin_amdgcn_logf(__builtin_amdgcn_exp2f(a - m) + __builtin_amdgcn_exp2f(b - m) +
                                     __builtin_amdgcn_exp2f(c - m));
}

// value of register r at lane-1 (state s-1), across the register boundary.
__device__ __forceinline__ float shift_up1(const float* a, int r, int lane) {
    float v = __shfl_up(a[r], 1, 64);
    float w = __shfl(a[r > 0 ? r - 1 : 0], 63, 64);
    return lane == 0 ? (r > 0 ? w : -INFINITY) : v;
}
__device__ __forceinline__ float shift_up2(const float* a, int r, int lane) {
    float v = __shfl_up(a[r], 2, 64);
    float w = __shfl(a[r > 0 ? r - 1 : 0], 62 + lane, 64);
    return lane < 2 ? (r > 0 ? w : -INFINITY) : v;
}
__device__ __forceinline__ float shift_dn1(const float* a, int r, int R, int lane) {
    float v = __shfl_down(a[r], 1, 64);
    float w = __shfl(a[r + 1 < R ? r + 1 : r], 0, 64);
    return lane == 63 ? (r + 1 < R ? w : -INFINITY) : v;
}
__device__ __forceinline__ float shift_dn2(const float* a, int r, int R, int lane) {
    float v = __shfl_down(a[r], 2, 64);
    float w = __shfl(a[r + 1 < R ? r + 1 : r], lane - 62, 64);
    return lane >= 62 ? (r + 1 < R ? w : -INFINITY) : v;
}

// Whole-wave DPP shifts (GFX9 wave_shr:1 / wave_shl:1): lane i takes lane i-1
// (resp. i+1); the lane shifted in gets -inf. Used when the lattice fits one
// register (S <= 64) instead of ds_bpermute shuffles on the recursion's
// critical path.
__device__ __forceinline__ float wave_shr1(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, -INFINITY),
                                                                 __builtin_bit_cast(int, v), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ float wave_shl1(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, -INFINITY),
                                                                 __builtin_bit_cast(int, v), 0x130, 0xf, 0xf, false));
}

// The frame part of the spotter's and the field reader's prep launches: one wave
// of a THREADS-wide workgroup per frame (b, t) writes rel = logit - max_c logit,
// a single float32 subtraction, into tab[b][t][c]. Frames at or past the row's
// length are neither read nor written.
template <int THREADS>
__device__ __forceinline__ void ctc_rel_frame(const float* __restrict__ logits, const int* __restrict__ seq_len, int T,
                                              int B, int C, float* __restrict__ tab) {
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
#pragma unroll
    for (int q = 0; q < NQ; ++q)
        if (lane + 64 * q < C) out[lane + 64 * q] = v[q] - m;
}

// A scoring workgroup's copy of its row's rel table [L][C] from the workspace into LDS rows of `stride`
// floats (stride == C: the table as it is; the keyed field reader appends its entry values to each row).
template <int THREADS>
__device__ __forceinline__ void ctc_tab_to_lds(const float* __restrict__ tab_b, float4* lds4, int L, int C,
                                               int stride) {
    if ((C & 3) == 0 && (stride & 3) == 0) {               // rows of whole float4s: tab_b is 16-B aligned
        const float4* src = reinterpret_cast<const float4*>(tab_b);
        if (stride == C) {
            for (int i = threadIdx.x; i < ((L * C) >> 2); i += THREADS) lds4[i] = src[i];
        } else {
            const int c4 = C >> 2, s4 = stride >> 2;
            for (int i = threadIdx.x; i < L * c4; i += THREADS) lds4[(i / c4) * s4 + i % c4] = src[i];
        }
    } else {
        float* dst = reinterpret_cast<float*>(lds4);
        if (stride == C) {
            for (int i = threadIdx.x; i < L * C; i += THREADS) dst[i] = tab_b[i];
        } else {
            for (int i = threadIdx.x; i < L * C; i += THREADS) dst[(i / C) * stride + i % C] = tab_b[i];
        }
    }
}

// ===================================================================== the keyword spotter's lattice
// (ctc_spot.hip has the account of the launch structure and the measurements behind these numbers)
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

// One keyword's check, with no row in sight: the status code (0 ok, 2 bad length, 3 bad label or alternative)
// and in req the frames it needs (n + the adjacent positions whose label sets overlap), -1 when it is not
// scored. A bad length never indexes the label rows; a bad label or alternative is only ever compared.
__device__ __forceinline__ int spot_check_keyword(const int* __restrict__ kw, const int* __restrict__ kw_alt,
                                                  const int* __restrict__ kw_len, int k, int max_kw_len, int C,
                                                  int& req) {
    const int len = kw_len[k];
    req = -1;
    if (len < 1 || len > SPOT_MAX_LEN || len > max_kw_len) return 2;
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
    if (bad) return 3;
    req = len + reps;
    return 0;
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
// TRAIL: the lane of state S - 1 also stores (V[t][S - 1], its start) into
// trail[t] after every frame, one 8-byte store: the keyword's best placement
// ending exactly at frame t + 1, the value compared with the running best.
// Nothing is stored for a keyword with len 0.
template <bool LDS, bool ALT, bool PAIR, bool TRAIL>
__device__ __forceinline__ void spot_best(const float* __restrict__ tab, const int* __restrict__ lab,
                                          const int* __restrict__ alt, int len, int L, int C, float2* trail,
                                          float& score, int& first, int& end) {
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
        if constexpr (TRAIL) {
            if (s == S - 1) trail[t] = make_float2(V, __int_as_float(st));
        }
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

// grid (chunks of SPOT_KW keywords) x B, SPOT_THREADS threads, T C floats of dynamic LDS when LDS.
// TRAIL: instead of score and span (not touched) every scored keyword's per-frame trail goes to
// trail[b][k][t] (t < L); a keyword that is not scored on the row (kinfo[k] < 0 or > L) leaves its
// trail unwritten, and its readers test kinfo the same way.
template <bool LDS, bool ALT, bool TRAIL>
__global__ void __launch_bounds__(SPOT_THREADS)
spot_score_kernel(const float* __restrict__ tab_g, const int* __restrict__ seq_len, int T, int C,
                  const int* __restrict__ kw, const int* __restrict__ kw_alt, const int* __restrict__ kw_len,
                  const int* __restrict__ kinfo, int n_kw, int max_kw_len, float* __restrict__ score,
                  int* __restrict__ span, float2* __restrict__ trail) {
    extern __shared__ float4 s_dyn4[];                     // LDS: the row's table, [L][C]
    const int b = blockIdx.y;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int L = min(max(seq_len[b], 0), T);
    const int k0 = blockIdx.x * SPOT_KW;
    float* out_v = score + (size_t)b * n_kw;
    int2* out_s = reinterpret_cast<int2*>(span) + (size_t)b * n_kw;
    const float* tab_b = tab_g + (size_t)b * T * C;
    float2* trail_b = TRAIL ? trail + (size_t)b * n_kw * T : nullptr;

    // a chunk with nothing to score (every keyword too long for this row, or not valid; L == 0)
    bool feasible = false;
    if (threadIdx.x < SPOT_KW && k0 + (int)threadIdx.x < n_kw) {
        const int req = kinfo[k0 + threadIdx.x];
        feasible = req >= 0 && req <= L;                   // req >= 1: never with L == 0
    }
    if (!__syncthreads_or(feasible)) {
        if constexpr (!TRAIL) {
            if (threadIdx.x < SPOT_KW && k0 + (int)threadIdx.x < n_kw) {
                out_v[k0 + threadIdx.x] = -INFINITY;
                out_s[k0 + threadIdx.x] = make_int2(-1, -1);
            }
        }
        return;
    }
    const float* tab = tab_b;
    if constexpr (LDS) {
        ctc_tab_to_lds<SPOT_THREADS>(tab_b, s_dyn4, L, C, C);   // <= T C floats = the launch's dynamic LDS
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
                spot_best<LDS, ALT, true, TRAIL>(tab, kw + (size_t)min(kh, n_kw - 1) * max_kw_len,
                                                 ALT ? kw_alt + (size_t)min(kh, n_kw - 1) * max_kw_len : nullptr,
                                                 h ? len[1] : len[0], L, C,
                                                 TRAIL ? trail_b + (size_t)min(kh, n_kw - 1) * T : nullptr, v, f, e);
            if constexpr (!TRAIL) {
                if ((lane & 31) == 0 && kh < n_kw) {
                    out_v[kh] = v;
                    out_s[kh] = make_int2(f, e);
                }
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
                spot_best<LDS, ALT, false, TRAIL>(tab, kw + (size_t)kh * max_kw_len,
                                                  ALT ? kw_alt + (size_t)kh * max_kw_len : nullptr, n, L, C,
                                                  TRAIL ? trail_b + (size_t)kh * T : nullptr, v, f, e);
            if constexpr (!TRAIL) {
                if (lane == 0) {
                    out_v[kh] = v;
                    out_s[kh] = make_int2(f, e);
                }
            }
        }
    }
}

// ===================================================================== the field reader's lattice
// (ctc_field.hip has the account of the launch structure)
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

// One pattern's check, with no row in sight: the status code (0 ok, 2 bad length or structure, 3 bad class)
// and in info its length and optional flags (len | mask << 8), -1 when it is not scored. A bad length never
// indexes the pattern's rows; a label is only ever compared.
__device__ __forceinline__ int field_check_pattern(const int* __restrict__ pat_cls, const int* __restrict__ pat_opt,
                                                   const int* __restrict__ pat_len, int p, int max_pat_len, int C,
                                                   int& info) {
    const int len = pat_len[p];
    info = -1;
    if (len < 1 || len > FIELD_MAX_LEN || len > max_pat_len) return 2;
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
    const int code = bad_structure ? 2 : bad_label ? 3 : 0;
    if (!code) info = len | (mask << 8);
    return code;
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
// ENTRY: what position 0 may be entered with at frame t. FIELD_ENTRY_FREE: float32 0, the free start.
// FIELD_ENTRY_TAB: the value behind the frame's table row, tab[t * stride + C + (the row's slot in the
// workgroup)]; FIELD_ENTRY_GAP: gap[goff + t].x from the workspace. Both are the keyed field reader's gap state
// G[t], fetched one frame ahead like the emissions and compared and added exactly where the free start's 0 is:
// the same expressions in the same order. stride is the table's row pitch in floats (C unless FIELD_ENTRY_TAB).
#define FIELD_ENTRY_FREE 0
#define FIELD_ENTRY_TAB 1
#define FIELD_ENTRY_GAP 2
template <int N, int ENTRY>
__device__ __forceinline__ void field_best(const float* __restrict__ tab, int stride, const int* __restrict__ cls,
                                           int info, int nmax, int L, int C, const float4* __restrict__ gap, int goff,
                                           float& score, int& first, int& end, int& label) {
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

    float Vs[N], Vb[N], en[N], enb, eng = 0.f;
    Pay Ps[N], Pb[N];
#pragma unroll
    for (int r = 0; r < N; ++r) {
        Vs[r] = Vb[r] = en[r] = -INFINITY;
        Ps[r] = Pb[r] = Pay{0u, 0u, 0u};
    }
    auto gather = [&](int t) {
        const float* row = tab + t * stride;
#pragma unroll
        for (int r = 0; r < N; ++r) {
            if (r < N - nmax) continue;
            const float e = row[max(lab[r], 0)];
            en[r] = lab[r] >= 0 ? e : -INFINITY;
        }
        enb = row[C - 1];
        if constexpr (ENTRY == FIELD_ENTRY_TAB) eng = row[C + ((int)threadIdx.x >> 4)];
        if constexpr (ENTRY == FIELD_ENTRY_GAP) eng = gap[goff + t].x;
    };
    float best_v = -INFINITY;
    int best_s = -1, best_e = -1;
    Pay best_p{0u, 0u, 0u};
    gather(0);
    for (int t = 0; t < L; ++t) {
        float e[N];
#pragma unroll
        for (int r = 0; r < N; ++r) e[r] = en[r];
        const float eb = enb, eg = eng;                      // eg: 0, or the gap state G[t]
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
            if (r == shift && eg > b) {                      // the free start: the filler before the hit scores 0
                b = eg;
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

// grid (chunks of FIELD_PAT patterns) x B, FIELD_THREADS threads, T C floats of dynamic LDS when LDS.
// KEYED (the keyed field reader, ctc_keyed.hip): pattern p is keyed field p; position 0 is entered with the gap
// state gap[b][p][t] = (value, keyword index, keyword first, keyword end) instead of 0 -- on the LDS route the
// values sit behind each table row, T (C + FIELD_PAT) floats of dynamic LDS -- span has four ints per result,
// (kw_first, kw_end, first, end), the keyword's read from gap[first], and kw_index and kw_score (the
// keyword's own value, trail[b][kw_index][kw_end - 1]) are written too.
template <bool LDS, bool KEYED>
__global__ void __launch_bounds__(FIELD_THREADS)
field_score_kernel(const float* __restrict__ tab_g, const int* __restrict__ seq_len, int T, int C,
                   const int* __restrict__ pat_cls, const int* __restrict__ pinfo, int n_pat, int max_pat_len,
                   float* __restrict__ score, int* __restrict__ span, int* __restrict__ text,
                   const float4* __restrict__ gap, const float2* __restrict__ trail, int n_kw,
                   int* __restrict__ kw_index, float* __restrict__ kw_score) {
    extern __shared__ float4 s_dyn4[];                     // LDS: the row's table, [L][C] ([L][C + FIELD_PAT] KEYED)
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
        constexpr int ENTRY = !KEYED ? FIELD_ENTRY_FREE : LDS ? FIELD_ENTRY_TAB : FIELD_ENTRY_GAP;
        const int stride = ENTRY == FIELD_ENTRY_TAB ? C + FIELD_PAT : C;
        // the workgroup's first field's gap states, and this DPP row's own field's offset from there
        const int p0 = blockIdx.x * FIELD_PAT;
        const float4* gap_b = KEYED ? gap + ((size_t)b * n_pat + p0) * T : nullptr;
        const int goff = (min(p, n_pat - 1) - p0) * T;
        if constexpr (LDS) {
            ctc_tab_to_lds<FIELD_THREADS>(tab_b, s_dyn4, L, C, stride);   // <= T stride floats = the dynamic LDS
            if constexpr (KEYED) {                         // slot q of frame t: G[t] of the workgroup's q-th field
                float* dst = reinterpret_cast<float*>(s_dyn4);
                for (int i = threadIdx.x; i < L * FIELD_PAT; i += FIELD_THREADS) {
                    const int q = i % FIELD_PAT, t = i / FIELD_PAT;
                    dst[t * stride + C + q] = p0 + q < n_pat ? gap_b[q * T + t].x : -INFINITY;
                }
            }
            __syncthreads();
            tab = reinterpret_cast<const float*>(s_dyn4);
        }
        // the wave's longest pattern picks the unrolling
        const int len = info & 255;
        const int nmax = max(max(__builtin_amdgcn_readlane(len, 0), __builtin_amdgcn_readlane(len, 16)),
                             max(__builtin_amdgcn_readlane(len, 32), __builtin_amdgcn_readlane(len, 48)));
        const int* cls = pat_cls + (size_t)min(p, n_pat - 1) * max_pat_len * FIELD_CLASS;
        if (nmax > 8) field_best<16, ENTRY>(tab, stride, cls, info, nmax, L, C, gap_b, goff, v, f, e, label);
        else if (nmax > 4) field_best<8, ENTRY>(tab, stride, cls, info, nmax, L, C, gap_b, goff, v, f, e, label);
        else if (nmax > 0) field_best<4, ENTRY>(tab, stride, cls, info, nmax, L, C, gap_b, goff, v, f, e, label);
    }
    if (p >= n_pat) return;
    const size_t o = (size_t)b * n_pat + p;
    if constexpr (KEYED) {
        if (lane16 == 0) {
            int4 sp = make_int4(-1, -1, f, e);
            int ki = -1;
            float kv = -INFINITY;
            if (f >= 0) {                                  // the gap state the hit entered with names its keyword
                const float4 g = gap[((size_t)b * n_pat + p) * T + f];
                ki = __float_as_int(g.y);
                sp.x = __float_as_int(g.z);
                sp.y = __float_as_int(g.w);
                kv = trail[((size_t)b * n_kw + ki) * T + sp.y - 1].x;
            }
            score[o] = v;
            reinterpret_cast<int4*>(span)[o] = sp;
            kw_index[o] = ki;
            kw_score[o] = kv;
        }
    } else if (lane16 == 0) {
        score[o] = v;
        reinterpret_cast<int2*>(span)[o] = make_int2(f, e);
    }
    for (int i = lane16; i < max_pat_len; i += 16) text[o * max_pat_len + i] = i < FIELD_MAX_LEN ? label : -1;
}
