// One-wave-per-SIMD MFMA engine for the large plain bf16 GEMMs (A_ROWK x B_NK,
// bf16 C, bias / ReLU epilogue): the calls gemm_pp.hip takes in A_ROWK mode --
// the recurrent input projections gx = x . W_x^T + b (model_bu.py:186-192) and
// their data gradients dx = dG . W_x.
//
// Geometry: a 256 x 256 x 64 tile per 256-thread workgroup, 4 waves as 2 x 2,
// one per SIMD; wave (wm, wn) owns the 128 x 128 output tile at rows wm*128,
// columns wn*128 as floatx4 acc[8][8] (256 accumulator registers; with
// __launch_bounds__(256) a wave has the 512-register budget). A K-tile is
// consumed as two k-blocks of 32 (kk = 0, 1); the fragments of a k-block (8 A +
// 8 B ds_read_b128, 64 registers) are double-buffered in registers, so the 64
// MFMAs of one k-block run while the 16 reads of the next are in flight.
// Against the ping-pong engine the workgroup reads 128 KB of LDS per K-tile
// instead of 192 KB (four 128 x 128 wave tiles instead of eight 128 x 64) and
// passes 2 barriers per K-tile instead of 8.
//
// LDS (149 KB): two 64-KB K-tile buffers with gemm_pp's image (A rows then B
// rows, 128 B per row, lane-linear 1-KB DMA pieces of 8 rows, the 16-B chunk
// XOR-swizzled by row & 7 on the global side, so every ds_read_b128 is
// conflict-free), staged as two 32-KB units per K-tile: UA = the 256 A rows,
// UB = the 256 B rows, 8 LDS-DMA pieces per wave each. The two-buffer form
// was chosen over a ring of 32-KB half-tiles because a k-block reads every
// row of the image (a k-half of a 128-B row is not a DMA unit of this image),
// and because the remaining 21 KB then hold a per-wave epilogue staging area
// and four bias slots, so the epilogue never touches a K-tile buffer and the
// staging DMAs run on across item boundaries.
// The DMA is the inline-asm form (lds_dma16_asm's instruction, with the
// piece's first row in the scalar offset): the fragment reads and the DMA
// pieces of this schedule sit inside the MFMA clusters, and a waitcnt pass
// that saw the DMAs would drain them (vmcnt(0)) in front of the next read.
//
// Schedule, K-tile s of the workgroup's stream (buffer s & 1), all four waves
// in step (no staggered groups):
//     K0(s):   64 MFMAs on kk = 0 | the 16 reads of kk = 1 of tile s
//     P(s):    lgkmcnt(0), vmcnt -> UA(s+1) landed, s_barrier
//     K1a(s):  32 MFMAs on kk = 1 | the 8 A reads of kk = 0 of tile s+1
//              | UA(s+2) into buffer s & 1, one piece per 4 MFMAs
//     M(s):    vmcnt -> UB(s+1) landed, s_barrier
//     K1b(s):  32 MFMAs on kk = 1 | the 8 B reads of kk = 0 of tile s+1 | UB(s+2)
// With one wave per SIMD nothing else hides a wave's address arithmetic, so
// the reads (sched_group_barrier in K0) and the DMA pieces (a sched_barrier
// per group of 4 MFMAs in K1a / K1b) are placed between the MFMAs.
// One barrier per staged unit; each is the unit's RAW barrier and P is also
// the WAR barrier:
//  * RAW: every wave waits (counted vmcnt, from a tally of the VMEM operations
//    it has issued, so epilogue stores, the bias piece and item boundaries
//    need no special cases) for its own pieces of UA(s+1) before barrier P(s)
//    and of UB(s+1) before M(s); the first reads of UA(s+1) are in K1a(s), of
//    UB(s+1) in K1b(s): the segment after the barrier that follows the wait.
//    In steady state UB(s+1) (8 pieces) stays in flight across P(s) and
//    UA(s+2) (8) across M(s): vmcnt is never 0 in the loop. A unit has two
//    k-blocks (one K-tile of MFMA time) to land.
//  * WAR: UA / UB(s+2) overwrite buffer s & 1 after P(s). Its last reads are
//    the kk = 1 reads of tile s, issued in K0(s); they are the only LDS reads
//    outstanding at P(s) (the reads of K1b(s-1) were consumed by K0(s)'s
//    MFMAs), so the counted wait that retires them is lgkmcnt(0) -- once per
//    K-tile, in front of the MFMAs that consume exactly those fragments. Inside
//    the clusters the compiler's counted lgkmcnt waits order each MFMA behind
//    the fragments it consumes only.
//  * Item boundary (persistent workgroups, one per CU for every K): the stream
//    of K-tiles runs across items, so the first two K-tiles of the next item
//    are staged under the current item's last ones. The epilogue runs after
//    K1b of an item's last K-tile out of registers through the wave's own
//    staging area (16 rows x 128 columns bf16 per slice, 8 slices,
//    wave_barrier only); its 32 stores per lane enter the tally. The bias of
//    an item (256 floats) is one more DMA piece in front of UB of the item's
//    first K-tile, issued by wave 0 into slot (item & 3) -- up to three items
//    are in flight when K = 64 -- and so landed and published by the barrier
//    that publishes that UB. Past the stream's end the pieces are all out of
//    range (zeros into a buffer nothing reads), so the clusters are
//    branch-free; a final vmcnt(0) lands them before the LDS is released.
//
// The MFMA operands are (B fragment, A fragment) with ascending k-blocks, as in
// gemm_pp: every output element accumulates the same f32 sequence, and the
// epilogue applies the same expression, so the result is bit-identical to
// gemm_pp's.
#include "gemm.h"
#include "mfma_util.h"

namespace ocrk {

namespace {

// NR x {NM MFMAs, 1 LDS read}, then the cluster's remaining MFMAs
template <int NR, int NM, int REST>
__device__ __forceinline__ void w4_interleave() {
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        __builtin_amdgcn_sched_group_barrier(0x8, NM, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
    }
    __builtin_amdgcn_sched_group_barrier(0x8, REST, 0);
}

typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));

// uniform_rsrc_words for operands that are uniform by construction (kernel arguments and the
// workgroup's item) and a byte count the launcher has checked to be < 2^31: no readfirstlane
// (its VGPR copies were hoisted out of the K loop and spilled), no 64-bit clamp
__device__ __forceinline__ i32x4_t w4_rsrc(const void* base, int bytes) {
    const uint64_t b = (uint64_t)base;
    return i32x4_t{(int)(unsigned)b, (int)((unsigned)(b >> 32) & 0xffffu), bytes, 0x00020000};
}

// BN = 256: the geometry above. BN = 128, for calls whose 256 x 256 items would leave half of the
// CUs idle: a 256 x 128 tile, the waves still 2 x 2, each a 128 x 64 tile (acc[8][4]); UB is 128
// rows (4 pieces per wave), a K-tile buffer 48 KB, the clusters half as many MFMAs around the
// same barriers (K0: 32 | 12 reads, K1a: 16 | 8 A reads | UA, K1b: 16 | 4 B reads | UB). Two
// buffers as well: a ring of three (144 KB, staged three K-tiles ahead) measured the same on the
// layer-1 data gradient, 89.6-93.5 against 91.9-93.6 us (profiles/w4conv_gemm_bench.txt; both
// with the accumulator shuffling that profiles/w4acc_isa.txt describes still in the K loop).
template <int BN>
__global__ void __launch_bounds__(256) gemm_w4_kernel(const GemmParams p) {
    constexpr int BM = 256, BK = 64, ROWB = 128;
    constexpr int WN = BN / 2, NJ = WN / 16;              // wave tile: 128 rows x WN columns, NJ B fragments
    constexpr int A_BYTES = BM * ROWB, BUF = (BM + BN) * ROWB;
    constexpr int NU = 8, NUB = BN / 32;                  // DMA instructions per wave per unit (UA, UB)
    constexpr int NB = 2;                                 // K-tile buffers (tile s in buffer s & 1)
    constexpr int BIAS_OFF = NB * BUF, STG_OFF = BIAS_OFF + 4 * 1024;
    constexpr int PITCH = WN * 2 + 16, STG = 16 * PITCH;  // staging: 16 rows x WN columns per wave
    constexpr int CL = WN / 8, RPS = 64 / CL;             // lanes per staged row, rows per store instruction
    constexpr int NST = 8 * (16 / RPS);                   // 16-B C stores per lane per item
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int i16 = lane & 15, g = lane >> 4, sw = lane & 7;

    // ---- this workgroup's items, XCD-contiguous as in gemm_pp
    const int tm = (p.M + BM - 1) / BM, tn = (p.N + BN - 1) / BN;
    const int nitems = tm * tn * p.batch;
    const int per = (nitems + 7) >> 3;
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, sp = gridDim.x >> 3;
    const int wend = min(nitems, (xcd + 1) * per);
    int w_issue = xcd * per + slot;
    if (w_issue >= wend) return;

    // arguments used once per item are re-read from the kernel-argument segment where they are
    // used (through a laundered pointer), not held in SGPRs across the K loop
    typedef const __attribute__((address_space(4))) GemmParams* KArgs;
    const bool has_bias = p.bias != nullptr;
    const int c_nk = max(1, (p.K + BK - 1) / BK);         // K-tiles per item (K = 0: one zero tile)

    // ---- issue side: the item whose K-tiles are being staged
    const int lrow = lane >> 3;
    const int cs = (lane & 7) ^ lrow;                     // global 16-B chunk this lane fetches
    i32x4_t ra, rb;
    int i_m0 = 0, i_n0 = 0, i_zb = 0, i_kt = 0, i_cnt = 0;
    const unsigned a_lane = (unsigned)(lrow * p.lda * 2), b_lane = (unsigned)(lrow * p.ldb * 2);
    auto setup_issue = [&](int w) {
        const PPItem it = pp_item(w, tm, tn, 1, BM, BN);
        ra = w4_rsrc(reinterpret_cast<const bf16*>(p.A) + it.zb * p.strideA, p.M * (int)p.lda * 2);
        rb = w4_rsrc(reinterpret_cast<const bf16*>(p.B) + it.zb * p.strideB, p.N * (int)p.ldb * 2);
        i_m0 = it.m0;
        i_n0 = it.n0;
        i_zb = it.zb;
        i_kt = 0;
    };
    int ops = 0;                                          // VMEM operations this wave has issued (uniform)
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
    // A unit's pieces share one per-lane offset (the lane's row of an 8-row piece and its 16-B
    // chunk of the K-tile; out of range past K or past the stream's end: zero fill); the piece's
    // first row goes into the instruction's scalar offset, so a piece costs a compare, a select
    // and three scalar operations among the MFMAs
    auto lane_off = [&](unsigned lane_row, bool on) -> unsigned {
        const int k = i_kt * BK + 8 * cs;
        return on && k < p.K ? lane_row + (unsigned)(k * 2) : W4_OOB;
    };
    // (the wave's first row and LDS address are laundered once per unit, so each piece is that
    // base plus an immediate, not 16 loop-invariant SGPRs)
    auto unit_base = [&](int first, unsigned buf, int& row, unsigned& lds) {
        row = first + wave * 8;
        lds = buf + wave * 8 * ROWB;
        asm volatile("" : "+s"(row), "+s"(lds));
    };
    auto dma_a = [&](int i, int row, unsigned lds, unsigned va) {
        const int mrow = row + i * 32;                    // uniform first row of the 8-row piece
        // rows past M: every lane is out of range, and the scalar offset stays inside the buffer
        const unsigned soff = mrow < p.M ? (unsigned)(mrow * (int)p.lda * 2) : 0u;
        w4_dma16(ra, lds + i * 32 * ROWB, lrow < p.M - mrow ? va : W4_OOB, soff);
    };
    auto dma_b = [&](int i, int row, unsigned lds, unsigned vb) {
        const int ncol = row + i * 32;
        const unsigned soff = ncol < p.N ? (unsigned)(ncol * (int)p.ldb * 2) : 0u;
        w4_dma16(rb, lds + i * 32 * ROWB, lrow < p.N - ncol ? vb : W4_OOB, soff);
    };
    // the item's bias (floats n0 + 4 lane .. + 3) in front of UB of the item's first K-tile
    auto dma_bias = [&](bool on) {
        if (i_kt == 0 && has_bias && wave == 0) {
            const int n = i_n0 + 4 * lane;
            KArgs e = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();
            asm volatile("" : "+s"(e));
            const i32x4_t rbias = w4_rsrc(e->bias + i_zb * e->strideBias, p.N * 4);
            w4_dma16(rbias, lds0 + BIAS_OFF + (i_cnt & 3) * 1024, on && 4 * lane < BN && n < p.N ? (unsigned)(n * 4) : W4_OOB, 0u);
            ops += 1;
        }
    };
    // after both units of a K-tile: the next K-tile, or the next item's first
    auto advance_issue = [&]() -> bool {
        if (++i_kt < c_nk) return true;
        w_issue += sp;
        ++i_cnt;
        if (w_issue >= wend) return false;
        setup_issue(w_issue);
        return true;
    };

    // ---- compute side
    int w_comp = w_issue, c_cnt = 0;

    bf16x8 af0[8], bf0[NJ], af1[8], bf1[NJ];              // fragments of kk = 0 / kk = 1
    const int a_base = (wm * 128 + i16) * ROWB, b_base = A_BYTES + (wn * WN + i16) * ROWB;
    auto read_a = [&](const char* buf, int kk, bf16x8 (&fr)[8]) {
#pragma unroll
        for (int i = 0; i < 8; ++i)
            fr[i] = *reinterpret_cast<const bf16x8*>(buf + a_base + i * 16 * ROWB + (((kk * 4 + g) ^ sw) << 4));
    };
    auto read_b = [&](const char* buf, int kk, bf16x8 (&fr)[NJ]) {
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            fr[j] = *reinterpret_cast<const bf16x8*>(buf + b_base + j * 16 * ROWB + (((kk * 4 + g) ^ sw) << 4));
    };
    floatx4 acc[8][NJ];
    (void)read_b;

    // ---- prologue: K-tiles 0 .. NB-1 of the stream; tile 0 landed, its kk = 0 fragments read
    int mA[NB + 1] = {}, mB[NB + 1] = {};                 // [d]: tallies behind UA / UB of tile s+d
    setup_issue(w_issue);
    bool more = true;
#pragma unroll
    for (int t = 0; t < NB; ++t) {
        const unsigned va = lane_off(a_lane, more), vb = lane_off(b_lane, more);
        int row;
        unsigned lds;
        unit_base(i_m0, lds0 + t * BUF, row, lds);
#pragma unroll
        for (int i = 0; i < NU; ++i) dma_a(i, row, lds, va);
        ops += NU;
        mA[t] = ops;
        dma_bias(more);
        unit_base(i_n0, lds0 + t * BUF + A_BYTES, row, lds);
#pragma unroll
        for (int i = 0; i < NUB; ++i) dma_b(i, row, lds, vb);
        ops += NUB;
        mB[t] = ops;
        if (more) more = advance_issue();
    }
    vm_wait_n(ops - mB[0]);
    w4_barrier();
    read_a(smem, 0, af0);
    read_b(smem, 0, bf0);

    int s = 0;
    // one K-tile of the stream. FIRST: the item's first K-tile, whose K0 MFMAs take the literal 0
    // as C (fma(a, b, +0) is what a zeroed accumulator computed), so an item's accumulators are
    // defined by their first MFMA -- no zeroing pass, and no value merged into the accumulator
    // registers at the item boundary for the register allocator to shuffle around
    auto k_tile = [&](auto FIRST_) {
        constexpr bool FIRST = decltype(FIRST_)::value;
        char* cur = smem + (s & 1) * BUF;
        const char* nxt = smem + ((s + 1) & 1) * BUF;
        // ---- K0: kk = 0 of tile s | reads of kk = 1
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
        read_a(cur, 1, af1);
        read_b(cur, 1, bf1);
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                if constexpr (FIRST)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf0[j], af0[i], floatx4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                else acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf0[j], af0[i], acc[i][j], 0, 0, 0);
            }
        if constexpr (NJ == 8) w4_interleave<16, 3, 16>();    // 64 MFMAs | 16 reads
        else w4_interleave<12, 2, 8>();                       // 32 MFMAs | 12 reads
        __builtin_amdgcn_s_setprio(0);
        // ---- P: tile s fully read (WAR), UA(s+1) landed (RAW)
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        vm_wait_fast<NUB>(ops - mA[1]);                       // UB(s+1) stays in flight
        w4_barrier();
        // ---- K1a: kk = 1, acc rows 0-3 | A reads of tile s+1 | UA(s+2) into buffer s & 1
        // (past the stream's end the reads return stale bytes that nothing consumes, and the
        // pieces are all out of range: zeros into a buffer that nothing reads)
        {
            const unsigned va = lane_off(a_lane, more);
            int row;
            unsigned lds;
            unit_base(i_m0, lds0 + (s & 1) * BUF, row, lds);
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                af0[q] = *reinterpret_cast<const bf16x8*>(nxt + a_base + q * 16 * ROWB + ((g ^ sw) << 4));
#pragma unroll
                for (int t = q * (NJ / 2); t < (q + 1) * (NJ / 2); ++t)   // NJ / 2 of the 4 NJ MFMAs per read
                    acc[t / NJ][t % NJ] =
                        __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf1[t % NJ], af1[t / NJ], acc[t / NJ][t % NJ], 0, 0, 0);
                dma_a(q, row, lds, va);
                __builtin_amdgcn_sched_barrier(0);
            }
            __builtin_amdgcn_s_setprio(0);
            ops += NU;
            mA[NB] = ops;
        }
        // ---- M: UB(s+1) landed
        vm_wait_fast<NU>(ops - mB[1]);                        // UA(s+2) stays in flight
        w4_barrier();
        // ---- K1b: kk = 1, acc rows 4-7 | B reads of tile s+1 | UB(s+2)
        {
            const unsigned vb = lane_off(b_lane, more);
            dma_bias(more);
            int row;
            unsigned lds;
            unit_base(i_n0, lds0 + (s & 1) * BUF + A_BYTES, row, lds);
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int q = 0; q < NJ; ++q) {
                bf0[q] = *reinterpret_cast<const bf16x8*>(nxt + b_base + q * 16 * ROWB + ((g ^ sw) << 4));
#pragma unroll
                for (int t = q * 4; t < q * 4 + 4; ++t)       // 4 of the 4 NJ MFMAs per read
                    acc[4 + t / NJ][t % NJ] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf1[t % NJ], af1[4 + t / NJ],
                                                                                      acc[4 + t / NJ][t % NJ], 0, 0, 0);
                dma_b(q, row, lds, vb);
                __builtin_amdgcn_sched_barrier(0);
            }
            __builtin_amdgcn_s_setprio(0);
            ops += NUB;
            mB[NB] = ops;
        }
        if (more) more = advance_issue();
        mA[1] = mA[2];
        mB[1] = mB[2];
        ++s;
    };

    for (;;) {                                            // items
        k_tile(std::true_type{});
        for (int c_kt = 1; c_kt < c_nk; ++c_kt) k_tile(std::false_type{});

        // ================================================= item epilogue
        {
            // lane geometry re-derived here: kept live across the K loop it costs the loop registers
            int el;                                           // the lane id (volatile: not hoisted)
            asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(el));
            const PPItem cur_it = pp_item(w_comp, tm, tn, 1, BM, BN);
            // the epilogue's arguments re-read from the kernel-argument segment, likewise
            KArgs e = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();
            asm volatile("" : "+s"(e));
            const int i16 = el & 15, g = el >> 4;
            // bias (the item's LDS slot: 0 past N; zeros without bias)
            const char* bslot = smem + BIAS_OFF + (c_cnt & 3) * 1024 + (wn * WN + 4 * g) * 4;
            floatx4 bv[NJ];
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                bv[j] = floatx4{0.f, 0.f, 0.f, 0.f};
                if (has_bias) bv[j] = *reinterpret_cast<const floatx4*>(bslot + j * 64);
            }
            // bf16 C through the wave's staging area, 16 rows per slice: each store
            // instruction writes RPS rows x 2 WN bytes at 16 B per lane
            char* stg = smem + STG_OFF + wave * STG;
            bf16* Cb = reinterpret_cast<bf16*>(e->C) + cur_it.zb * e->strideC;
            const __amdgpu_buffer_rsrc_t rc =
                __builtin_amdgcn_make_buffer_rsrc(Cb, 0, ((p.M - 1) * (int)e->ldc + p.N) * 2, 0x00020000);
            const int c8 = el & (CL - 1), r0 = el / CL;
            const int n = cur_it.n0 + wn * WN + 8 * c8;
#pragma unroll
            for (int h = 0; h < 8; ++h) {
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    floatx4 v = acc[h][j] * e->alpha + bv[j];          // gemm_pp's epilogue expression
                    if (e->relu) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
                    }
                    u16x4 o;
#pragma unroll
                    for (int r = 0; r < 4; ++r) o[r] = __builtin_bit_cast(unsigned short, (bf16)v[r]);
                    *reinterpret_cast<u16x4*>(stg + i16 * PITCH + (j * 16 + 4 * g) * 2) = o;
                }
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int q = 0; q < 16 / RPS; ++q) {
                    const int r = r0 + q * RPS;
                    const int m = cur_it.m0 + wm * 128 + h * 16 + r;
                    const u32x4 v = *reinterpret_cast<const u32x4*>(stg + r * PITCH + c8 * 16);
                    const unsigned off = (m < p.M && n < p.N) ? (unsigned)(((int64_t)m * e->ldc + n) * 2) : W4_OOB;
                    __builtin_amdgcn_raw_buffer_store_b128(v, rc, off, 0, 0);
                }
                __builtin_amdgcn_wave_barrier();
            }
            ops += NST;
        }
        w_comp += sp;
        ++c_cnt;
        if (w_comp >= wend) break;
    }
    vm_wait<0>();                                         // the zero-fill pieces past the stream's end land before the LDS is released
}

}  // namespace

// Runs the one-wave-per-SIMD engine when GEMM_W4 routes the call to it; -1 otherwise.
int gemm_w4(const GemmParams& p, int amode, int bmode, int dtype, hipStream_t stream) {
    const int64_t mode = opt(OPT_GEMM_W4);
    if (mode == 0 || dtype != OCRK_BF16 || amode != A_ROWK || bmode != B_NK) return -1;
    // gemm_pp's A_ROWK preconditions: bf16 C, whole K per item, no mask / stats
    if (!p.c_bf16 || p.accumulate || p.splits != 1 || p.mask || p.stats || p.mask_bits || p.relu_bits) return -1;
    if (p.N % 8 != 0 || p.K % 8 != 0 || (int64_t)p.M < 4096 || p.N < 96) return -1;
    if ((int64_t)p.M * p.lda * 2 >= (1ll << 31) || (int64_t)p.N * p.ldb * 2 >= (1ll << 31) ||
        (int64_t)p.M * p.ldc * 2 >= (1ll << 31))
        return -1;
    if (p.ldc % 8 != 0 || p.strideC % 8 != 0 || (uintptr_t)p.C % 16 != 0) return -1;
    if (p.bias && (uintptr_t)p.bias % 16 != 0) return -1;
    if (p.lda % 8 != 0 || p.ldb % 8 != 0) return -1;
    // GEMM_W4=1, the measured routes: K >= 1024 and N >= 256 -- both data gradients and the layer-2
    // projection (profiles/w4acc_gemm_bench.txt, us, fastest-slowest of 5 interleaved repetitions,
    // ping-pong / NT ring -> this engine; a shape is won if this engine's slowest repetition beats
    // the other's fastest):
    //   dx L2     32000 x 1024 x 4096   231.0-238.4 -> 209.0-219.2   won
    //   proj L2   32000 x 4096 x 1024   260.5-318.8 -> 227.6-253.5   won
    //   dx L1     32000 x 256 x 4096     80.8-83.2  ->  71.6-72.5    won (256 x 128 tile, 250 items; NT ring)
    //   proj L1   32000 x 4096 x 256     96.0-109.4 ->  87.7-97.5    ranges overlap: not routed
    //   logits dx 32000 x 1024 x 96      21.7-21.9  ->  21.1-21.2    won by 0.5 us, short K: not routed
    // (before the K loops accumulated in place -- profiles/w4acc_isa.txt -- proj L2 overlapped,
    // 266.5-330.9 -> 252.0-278.2, and dx L1 lost, 80.8-82.7 -> 91.9-93.6: profiles/w4_gemm_bench.txt,
    // w4conv_gemm_bench.txt)
    // 2: every covered shape
    if (mode == 1 && (p.K < 1024 || p.N < 256)) return -1;
    const int ncu = cu_count();
    // the 256 x 128 tile where 256 x 256 items would cover at most half of the CUs (one round
    // either way, of items half as long)
    const bool narrow = 2 * cdiv(p.M, 256) * cdiv(p.N, 256) * (int64_t)p.batch <= ncu;
    const int bn = narrow ? 128 : 256;
    const int lds = 2 * (256 + bn) * 128 + 4 * 1024 + 4 * 16 * (bn + 16);
    static DeviceOnce configured[2];
    const void* kern = narrow ? reinterpret_cast<const void*>(&gemm_w4_kernel<128>)
                              : reinterpret_cast<const void*>(&gemm_w4_kernel<256>);
    set_dyn_lds(configured[narrow ? 1 : 0], kern, lds);
    const int64_t items = cdiv(p.M, 256) * cdiv(p.N, bn) * (int64_t)p.batch;
    // persistent always (one workgroup per CU): the K-tile stream runs across items, so an item's
    // prologue is staged under the previous item's last K-tiles, and the epilogue's stores are in
    // the tally, never in front of a wait
    const int64_t grid = std::min<int64_t>(cdiv(items, 8) * 8, (int64_t)(ncu / 8) * 8);
    if (narrow) gemm_w4_kernel<128><<<dim3((unsigned)grid), 256, lds, stream>>>(p);
    else gemm_w4_kernel<256><<<dim3((unsigned)grid), 256, lds, stream>>>(p);
    opt_add(OPT_GEMM_W4_LAUNCHES, 1);
    return launch_status("gemm_w4");
}

}  // namespace ocrk
