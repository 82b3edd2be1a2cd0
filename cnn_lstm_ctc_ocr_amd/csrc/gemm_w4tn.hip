// One-wave-per-SIMD MFMA engine for the k-major ("TN") weight gradients, bf16
// operands, f32 C:
//   C[M,N] (+)= A^T . B,  A stored [K][lda] (A(m,k) = A[k*lda + m]),
//                         B stored [K][ldb] (B(k,n) = B[k*ldb + n])
// -- the calls gemm_pptn.hip takes in A_COLK mode: the recurrent and logits
// weight gradients dW = x^T dG, h_prev^T dG over the T*B time-major rows
// (model_bu.py:167-199 / model.py:216-220), K = T*B, batched over the two
// directions, split K into f32 partials (reduced by gemm.hip's splitk_finish).
// AM = A_IM2COL_T takes gemm_pptn's other mode on the same schedule: the conv
// weight gradient dW[(kh,kw,c)][cout] = im2col(x)^T . dy over the B*H*W pixels
// for Cin % 64 == 0 and Cout >= 256 (conv7, conv8), where the A operand is
// gathered from the NHWC input (see the A_IM2COL_T block in the kernel).
//
// The geometry and the schedule are gemm_w4.hip's (read it first): a 256 x 256
// x 64 tile per 256-thread workgroup, 4 waves as 2 x 2, one per SIMD, a 128 x
// 128 register tile (floatx4 acc[8][8]) per wave, the fragments of a 32-deep
// k-block double-buffered in registers, two 64-KB K-tile buffers staged as two
// 32-KB units (UA, UB; 8 LDS-DMA pieces per wave each), per K-tile kt:
//     K0:   64 MFMAs on kk = 0 | the 32 transposed reads of kk = 1
//     P:    lgkmcnt(0), vmcnt -> UA(kt+1) landed, s_barrier
//     K1a:  32 MFMAs on kk = 1 | 16 reads (A, kk = 0 of kt+1) | UA(kt+2), a piece per 4 MFMAs
//     M:    vmcnt -> UB(kt+1) landed, s_barrier
//     K1b:  32 MFMAs on kk = 1 | 16 reads (B, kk = 0 of kt+1) | UB(kt+2)
// with the same RAW / WAR arithmetic: a unit is waited for (counted vmcnt: the
// one unit issued after it stays in flight, 8 pieces) before the barrier in
// front of the segment that first reads it; UA / UB(kt+2) overwrite buffer
// kt & 1 after P(kt), behind the lgkmcnt(0) that retires the kk = 1 reads of
// K-tile kt, the only LDS reads outstanding there. Past the last K-tile the
// pieces are all out of range (zeros into a buffer nothing reads) and the
// fragment reads return stale bytes nothing consumes, so the loop body is
// branch-free; a vmcnt(0) in front of the epilogue lands them.
//
// Only the operand images differ, and they are gemm_pptn's: both operands are
// k-major, a unit is four [64 k][64 columns] bf16 blocks (128-B rows, 16-B
// chunk slot = chunk ^ (k & 7), swizzled on the global side), block b of A
// holding columns m0 + 64 b, of B columns n0 + 64 b; DMA piece i of a wave
// covers k-rows ((i & 1) * 4 + wave) * 8 .. + 8 of block i >> 1. The fragments
// come out with ds_read_b64_tr_b16 (frag_tr). The DMA is the inline-asm form
// for the reason given in DESIGN section 3.
// One work item (output tile x K slice x batch entry) per workgroup, as
// gemm_pptn: split K writes f32 partials, else C (+)= in place.
//
// The MFMA operands are (B fragment, A fragment) with ascending k-blocks and
// the epilogue is gemm_pptn's expression, so every output element is
// bit-identical to gemm_pptn's, split-K partials included.
#include "gemm.h"
#include "mfma_util.h"

namespace ocrk {

namespace {

template <int AM>
__global__ void __launch_bounds__(256) gemm_w4tn_kernel(const GemmParams p) {
    constexpr bool IM = AM == A_IM2COL_T;
    constexpr int BM = 256, BN = 256, BK = 64, ROWB = 128, BLK = BK * ROWB;   // 8-KB [64 k][64 col] block
    constexpr int A_BYTES = 4 * BLK, BUF = 8 * BLK;
    constexpr int NU = 8;                                 // DMA instructions per wave per unit
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int i16 = lane & 15, g = lane >> 4;

    // ---- the item: XCD-contiguous ranges as in gemm_pptn (one item per workgroup)
    const int tm = (p.M + BM - 1) / BM, tn = (p.N + BN - 1) / BN;
    const int nT = tm * tn;
    const int nitems = nT * p.batch * p.splits;
    const int per = (nitems + 7) >> 3;
    const int w = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
    if (w >= nitems || (int)(blockIdx.x >> 3) >= per) return;
    const int z = w / nT, t = w - z * nT;
    constexpr int GM = 4;
    const int gsz = GM * tn, grp = t / gsz, first = grp * GM;
    const int gm = min(GM, tm - first), rr = t - grp * gsz;
    const int m0 = (first + rr % gm) * BM, n0 = (rr / gm) * BN;
    const int zb = z / p.splits, zs = z - zb * p.splits;
    const int kbeg = zs * p.k_chunk;
    const int kend = min(p.K, kbeg + p.k_chunk);
    const int nk = max(1, (kend - kbeg + BK - 1) / BK);
    // descriptors from uniform words (kernel arguments and the item); byte counts < 2^31 (launcher)
    const uint64_t pa = (uint64_t)(reinterpret_cast<const bf16*>(p.A) + zb * p.strideA);
    const uint64_t pb = (uint64_t)(reinterpret_cast<const bf16*>(p.B) + zb * p.strideB);
    const i32x4_t ra = {(int)(unsigned)pa, (int)((unsigned)(pa >> 32) & 0xffffu),
                        p.K * (IM ? p.convC : (int)p.lda) * 2, 0x00020000};
    const i32x4_t rb = {(int)(unsigned)pb, (int)((unsigned)(pb >> 32) & 0xffffu), p.K * (int)p.ldb * 2, 0x00020000};

    // ---- per-lane DMA geometry: piece i (0..7) of a wave's unit is block i >> 1, k-rows
    // ((i & 1) * 4 + wave) * 8 + lane / 8, slot lane & 7. The lane's offset within the K-tile and
    // the block (k-row and 16-B chunk) is loop-invariant; the K-tile's first row and the block's
    // first column go into the instruction's scalar offset.
    const int lrow = lane >> 3;
    const int chunk = (lane & 7) ^ lrow;                  // global 16-B chunk of the row this lane fetches
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
    unsigned va[2], vb[2];
    int krow[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        krow[h] = (h * 4 + wave) * 8 + lrow;
        va[h] = IM ? (unsigned)((krow[h] * p.convC + 8 * chunk) * 2)
                   : (unsigned)((krow[h] * (int)p.lda + m0 + 8 * chunk) * 2);
        vb[h] = (unsigned)((krow[h] * (int)p.ldb + n0 + 8 * chunk) * 2);
    }
    // A_IM2COL_T (gemm_pptn's im2col A block): k is a pixel of the NHWC input and a 64-column block
    // is 64 channels of one tap (Cin % 64 == 0; tap and first channel uniform per item), so a k-row
    // of a block is 128 contiguous bytes at the shifted pixel, or zeros where the tap leaves the
    // image. Per block: the tap's bit (0 for a block past M) and the byte shift of its source.
    // Per lane: the two pixels (row ph, column pw) of the K-tile to be issued next, stepped by 64
    // pixels per K-tile without a division, and the 9-bit mask of their taps inside the image.
    // The whole source offset is per lane (no scalar part): alone, a tap's shift may be negative.
    unsigned t_bit[4] = {0, 0, 0, 0}, t_sh[4] = {0, 0, 0, 0};
    int pw[2] = {0, 0}, ph[2] = {0, 0};
    unsigned pmask[2] = {0, 0};
    int step_w = 0, step_h = 0;
    auto tap_mask = [&](int h) {
        const unsigned cb = 2u | (pw[h] > 0 ? 1u : 0u) | (pw[h] < p.convW - 1 ? 4u : 0u);
        pmask[h] = (cb << 3) | (ph[h] > 0 ? cb : 0u) | (ph[h] < p.convH - 1 ? cb << 6 : 0u);
    };
    if constexpr (IM) {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int col = min(m0 + 64 * b, p.M - 1);
            const int tap = col / p.convC;
            t_bit[b] = m0 + 64 * b < p.M ? 1u << tap : 0u;
            t_sh[b] = (unsigned)((((tap / 3 - 1) * p.convW + tap % 3 - 1) * p.convC + col - tap * p.convC) * 2);
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int k = kbeg + krow[h];
            pw[h] = k % p.convW;
            ph[h] = (k / p.convW) % p.convH;
            tap_mask(h);
        }
        step_w = BK % p.convW;
        step_h = (BK / p.convW) % p.convH;
    }
    auto next_pixels = [&]() {                            // after UA of a K-tile: the next K-tile's pixels
        if constexpr (IM) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                pw[h] += step_w;
                const bool wrap = pw[h] >= p.convW;
                pw[h] -= wrap ? p.convW : 0;
                ph[h] += step_h + (wrap ? 1 : 0);
                ph[h] -= ph[h] >= p.convH ? p.convH : 0;
                tap_mask(h);
            }
        }
    };
    // piece i of UA / UB of K-tile kt into the buffer at LDS address buf (on = false: all out of range)
    auto dma_a = [&](int i, int kt, unsigned buf, bool on) {
        const int k0 = kbeg + kt * BK;
        if constexpr (IM) {
            const int b = i >> 1, h = i & 1;
            // (& not &&: a select among the MFMAs, never a branch on the lane's mask)
            const bool ok = on & (k0 + krow[h] < kend) & ((pmask[h] & t_bit[b]) != 0);
            const unsigned base = (unsigned)(k0 * p.convC * 2) + t_sh[b];
            w4_dma16(ra, buf + b * BLK + (h * 4 + wave) * 1024, ok ? va[h] + base : W4_OOB, 0u);
            return;
        }
        const bool ok = on && k0 + krow[i & 1] < kend && m0 + 64 * (i >> 1) + 8 * chunk < p.M;
        const unsigned soff = on ? (unsigned)(k0 * (int)p.lda * 2 + 128 * (i >> 1)) : 0u;
        w4_dma16(ra, buf + (i >> 1) * BLK + ((i & 1) * 4 + wave) * 1024, ok ? va[i & 1] : W4_OOB, soff);
    };
    auto dma_b = [&](int i, int kt, unsigned buf, bool on) {
        const int k0 = kbeg + kt * BK;
        const bool ok = on && k0 + krow[i & 1] < kend && n0 + 64 * (i >> 1) + 8 * chunk < p.N;
        const unsigned soff = on ? (unsigned)(k0 * (int)p.ldb * 2 + 128 * (i >> 1)) : 0u;
        w4_dma16(rb, buf + A_BYTES + (i >> 1) * BLK + ((i & 1) * 4 + wave) * 1024, ok ? vb[i & 1] : W4_OOB, soff);
    };

    // ---- transposed fragment reads (frag_tr): lane reads k-row kr0 (+16) of the 32-deep k-block,
    // 4 consecutive columns at cq within a 16-column group
    const int kr0 = 4 * g + (i16 >> 2), cq = 4 * (i16 & 3);
    auto tr_off = [&](int blk, int col, int kk) {        // byte offset of (k-row kk*32 + kr0, col) in block blk
        const int r = kk * 32 + kr0;
        return blk * BLK + r * ROWB + ((((col >> 3) ^ (r & 7))) << 4) + (col & 7) * 2;
    };
    auto frag_a = [&](const char* buf, int i, int kk) {  // A fragment i: columns wm*128 + i*16 ..
        return frag_tr(reinterpret_cast<const unsigned short*>(buf + tr_off(2 * wm + (i >> 2), (i & 3) * 16 + cq, kk)),
                       16 * (ROWB / 2));
    };
    auto frag_b = [&](const char* buf, int j, int kk) {
        return frag_tr(reinterpret_cast<const unsigned short*>(
                           buf + A_BYTES + tr_off(2 * wn + (j >> 2), (j & 3) * 16 + cq, kk)),
                       16 * (ROWB / 2));
    };

    floatx4 acc[8][8];
    bf16x8 af0[8], bf0[8], af1[8], bf1[8];                // fragments of kk = 0 / kk = 1

    // ---- prologue: K-tiles 0 and 1; tile 0 landed, its kk = 0 fragments read
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2) {
#pragma unroll
        for (int i = 0; i < NU; ++i) dma_a(i, t2, lds0 + t2 * BUF, t2 < nk);
        next_pixels();
#pragma unroll
        for (int i = 0; i < NU; ++i) dma_b(i, t2, lds0 + t2 * BUF, t2 < nk);
    }
    vm_wait<2 * NU>();
    w4_barrier();
#pragma unroll
    for (int i = 0; i < 8; ++i) af0[i] = frag_a(smem, i, 0);
#pragma unroll
    for (int j = 0; j < 8; ++j) bf0[j] = frag_b(smem, j, 0);

    // one K-tile. FIRST: the item's first K-tile, whose K0 MFMAs take the literal 0 as C
    // (fma(a, b, +0) is what a zeroed accumulator computed): no zeroing pass
    auto k_tile = [&](auto FIRST_, int kt) {
        constexpr bool FIRST = decltype(FIRST_)::value;
        const char* cur = smem + (kt & 1) * BUF;
        const char* nxt = smem + ((kt + 1) & 1) * BUF;
        const unsigned curl = lds0 + (kt & 1) * BUF;
        const bool more = kt + 2 < nk;
        // ---- K0: kk = 0 of K-tile kt | reads of kk = 1
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int i = 0; i < 8; ++i) af1[i] = frag_a(cur, i, 1);
#pragma unroll
        for (int j = 0; j < 8; ++j) bf1[j] = frag_b(cur, j, 1);
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if constexpr (FIRST)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf0[j], af0[i], floatx4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                else acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf0[j], af0[i], acc[i][j], 0, 0, 0);
            }
#pragma unroll
        for (int r = 0; r < 24; ++r) {                    // 24 x {2 MFMAs, 1 read}, 8 x {1, 1}, 8 MFMAs
            __builtin_amdgcn_sched_group_barrier(0x8, 2, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x8, 8, 0);
        __builtin_amdgcn_s_setprio(0);
        // ---- P: K-tile kt fully read (WAR), UA(kt+1) landed (RAW; UB(kt+1) stays in flight)
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        vm_wait<NU>();
        w4_barrier();
        // ---- K1a: kk = 1, acc rows 0-3 | A reads of K-tile kt+1 | UA(kt+2) into buffer kt & 1
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            af0[q] = frag_a(nxt, q, 0);
#pragma unroll
            for (int j = (q & 1) * 4; j < (q & 1) * 4 + 4; ++j)
                acc[q >> 1][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf1[j], af1[q >> 1], acc[q >> 1][j], 0, 0, 0);
            dma_a(q, kt + 2, curl, more);
            __builtin_amdgcn_sched_barrier(0);
        }
        next_pixels();
        __builtin_amdgcn_s_setprio(0);
        // ---- M: UB(kt+1) landed (UA(kt+2) stays in flight)
        vm_wait<NU>();
        w4_barrier();
        // ---- K1b: kk = 1, acc rows 4-7 | B reads of K-tile kt+1 | UB(kt+2)
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            bf0[q] = frag_b(nxt, q, 0);
#pragma unroll
            for (int j = (q & 1) * 4; j < (q & 1) * 4 + 4; ++j)
                acc[4 + (q >> 1)][j] =
                    __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf1[j], af1[4 + (q >> 1)], acc[4 + (q >> 1)][j], 0, 0, 0);
            dma_b(q, kt + 2, curl, more);
            __builtin_amdgcn_sched_barrier(0);
        }
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
    };
    k_tile(std::true_type{}, 0);
    for (int kt = 1; kt < nk; ++kt) k_tile(std::false_type{}, kt);
    vm_wait<0>();                                         // the zero-fill pieces past the last K-tile

    // ---- epilogue: lane holds C[m][n .. n+3], m = m0 + wm*128 + i*16 + i16,
    // n = n0 + wn*128 + j*16 + 4g; f32 (+)= or split-K partials
    const int mrow0 = m0 + wm * 128 + i16, ncol0 = n0 + wn * 128 + 4 * g;
    float* C;
    int64_t ldc;
    bool acc_c;
    if (p.splits > 1) {
        C = p.splitk_ws + ((int64_t)zb * p.splits + zs) * (int64_t)p.M * p.N;
        ldc = p.N;
        acc_c = false;
    } else {
        C = reinterpret_cast<float*>(p.C) + zb * p.strideC;
        ldc = p.ldc;
        acc_c = p.accumulate != 0;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int m = mrow0 + i * 16;
        if (m >= p.M) continue;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int n = ncol0 + j * 16;
            if (n >= p.N) continue;
            floatx4* dst = reinterpret_cast<floatx4*>(C + (int64_t)m * ldc + n);
            floatx4 v = acc[i][j] * p.alpha;
            if (acc_c) v += *dst;
            *dst = v;
        }
    }
}

}  // namespace

// Runs the one-wave-per-SIMD TN engine when GEMM_W4 routes the call to it; -1 otherwise.
int gemm_w4tn(const GemmParams& p, int amode, int bmode, int dtype, hipStream_t stream) {
    const int64_t mode = opt(OPT_GEMM_W4);
    const bool im = amode == A_IM2COL_T;
    if (mode == 0 || dtype != OCRK_BF16 || (amode != A_COLK && !im) || bmode != B_KN) return -1;
    // gemm_pptn's preconditions (A_IM2COL_T: Cin % 64 == 0, one problem)
    if (!gemm_pptn_covers(amode, p.M, p.N, p.convC)) return -1;
    if (p.c_bf16 || p.bias || p.relu || p.mask || p.stats) return -1;
    if (p.ldb % 8 != 0 || (!im && p.lda % 8 != 0)) return -1;
    if (p.splits == 1 && (p.ldc % 4 != 0 || (uintptr_t)p.C % 16 != 0 || p.strideC % 4 != 0)) return -1;
    if (p.splits > 1 && (uintptr_t)p.splitk_ws % 16 != 0) return -1;
    // 32-bit source offsets (A_IM2COL_T: up to two K-tiles past K are formed, then discarded)
    const int64_t a_bytes = im ? ((int64_t)p.K + 128) * p.convC * 2 : (int64_t)p.K * p.lda * 2;
    if (a_bytes >= (1ll << 31) || (int64_t)p.K * p.ldb * 2 >= (1ll << 31)) return -1;
    if (im && (p.batch != 1 || p.convH < 1 || p.convW < 1 || p.M != 9 * p.convC)) return -1;
    // GEMM_W4=1, the measured route = every covered shape: each recurrent weight gradient won
    // (profiles/w4_gemm_bench.txt, us per direction incl. the split-K reduce, 5 interleaved
    // repetitions, ping-pong -> this engine): L2 dW_x 1024 x 2048 x 32000 151.4-174.1 -> 123.1-139.3,
    // dW_h 512 x 2048 91.8-102.5 -> 77.2-84.3, L1 dW_x 256 x 2048 57.9-60.7 -> 51.1-52.6;
    // and each im2col conv weight gradient at B = 256 (profiles/w4conv_gemm_bench.txt, us per call
    // incl. the split-K reduce): conv7 1152 x 256 x 96000 113.3-120.0 -> 80.2-83.8,
    // conv8 2304 x 256 x 96000 185.5-199.3 -> 125.2-132.2; with the im2col K loop accumulating in
    // place (profiles/w4acc_isa.txt, w4acc_gemm_bench.txt) conv7 112.6-122.3 -> 76.3-80.9,
    // conv8 184.8-200.6 -> 117.2-125.0, the recurrent gradients unchanged
    constexpr int LDS = 2 * 8 * 64 * 128;
    static DeviceOnce configured[2];
    const void* kern = im ? reinterpret_cast<const void*>(&gemm_w4tn_kernel<A_IM2COL_T>)
                          : reinterpret_cast<const void*>(&gemm_w4tn_kernel<A_COLK>);
    set_dyn_lds(configured[im ? 1 : 0], kern, LDS);
    const int64_t items = cdiv(p.M, 256) * cdiv(p.N, 256) * (int64_t)p.batch * p.splits;
    const dim3 grid((unsigned)(cdiv(items, 8) * 8));
    if (im) gemm_w4tn_kernel<A_IM2COL_T><<<grid, 256, LDS, stream>>>(p);
    else gemm_w4tn_kernel<A_COLK><<<grid, 256, LDS, stream>>>(p);
    opt_add(OPT_GEMM_W4_LAUNCHES, 1);
    return launch_status("gemm_w4tn");
}

}  // namespace ocrk
