// The extended-label lattice helpers shared by the CTC loss / alignment
// (ctc.hip) and the lexicon scorer (ctc_lexicon.hip): base-2 log-sum-exps and
// the state shifts of a lattice held in the registers of one wave (lane j
// holds states j, j + 64, ...: R registers); and the rel table of the keyword
// spotter (ctc_spot.hip) and the field reader (ctc_field.hip).
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
