// Page -> line crops on the device: what src/processing/pagepredictor.py:274,
// 319-328 does on the host with cv2 (min-max normalise the page, cut each line box, resize it
// to height 32, * 255 as uint8) and server.Bucket.addImgToBucket / fill_batch do in NumPy
// (zero-pad each crop to its bucket's width, top a short batch up with zero crops).
//
//   ocrk_page_minmax  min and max of a uint8 / f32 page into two floats in device memory
//   ocrk_page_crops   one launch for every crop of the page: a table of jobs (source
//                     rectangle, nw, bucket width, place in one flat uint8 arena), every
//                     byte of the arena written (samples, padding zeros, top-up crops)
//
// Sampling: cv2.resize(INTER_LINEAR)'s half-pixel-centre rule per axis. For destination
// index d of n over a source of s pixels, c = (d + 0.5) s / n - 0.5 = num / 2n is taken
// from integers: num = (2d + 1) s - n, i = num div 2n, f = (num - 2n i) / 2n (one rounding,
// of a quotient of two small integers), i < 0 -> (0, 0), i >= s - 1 -> (s - 1, 0). The box's
// y0 / x0 are added to i as integers, so the position inside a page costs no precision.
#include "common.h"

namespace {

// ------------------------------------------------------------------ min / max
// Order-preserving image of a float in an unsigned word: larger float <=> larger word. A zeroed
// word is below every float's image, so 0 is the identity of an unsigned atomic max; the minimum
// is kept as the maximum of the complemented image.
__device__ __forceinline__ unsigned f32_ordered(float x) {
    const unsigned u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float f32_unordered(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__device__ __forceinline__ float wave_min(float v) { return -wave_max(-v); }

template <typename T> struct Vec16;
template <> struct Vec16<float> {
    static constexpr int N = 4;
    static __device__ __forceinline__ void fold(const float* p, float& mn, float& mx) {
        const float4 v = *reinterpret_cast<const float4*>(p);
        mn = fminf(fminf(mn, v.x), fminf(v.y, fminf(v.z, v.w)));
        mx = fmaxf(fmaxf(mx, v.x), fmaxf(v.y, fmaxf(v.z, v.w)));
    }
};
template <> struct Vec16<uint8_t> {
    static constexpr int N = 16;
    static __device__ __forceinline__ void fold(const uint8_t* p, float& mn, float& mx) {
        const uint4 v = *reinterpret_cast<const uint4*>(p);
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
        unsigned lo = 255, hi = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int k = 0; k < 32; k += 8) {
                const unsigned b = (w[i] >> k) & 255u;
                lo = min(lo, b);
                hi = max(hi, b);
            }
        mn = fminf(mn, (float)lo);
        mx = fmaxf(mx, (float)hi);
    }
};

// ws: three zeroed words (ordered max, complemented ordered min, finished workgroups). `head`
// elements before the first 16-byte boundary and the tail after the last whole vector are
// read one by one; the body in 16-byte loads, grid-stride.
template <typename T>
__global__ void __launch_bounds__(256) page_minmax_kernel(const T* __restrict__ page, int64_t n, int head,
                                                          unsigned* __restrict__ ws, float* __restrict__ out) {
    constexpr int N = Vec16<T>::N;
    float mn = INFINITY, mx = -INFINITY;
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t nthreads = (int64_t)gridDim.x * 256;
    const int64_t nvec = (n - head) / N;
    const T* body = page + head;
    for (int64_t v = gid; v < nvec; v += nthreads) Vec16<T>::fold(body + v * N, mn, mx);
    const int64_t tail0 = head + nvec * N;
    for (int64_t i = gid; i < head; i += nthreads) {
        mn = fminf(mn, (float)page[i]);
        mx = fmaxf(mx, (float)page[i]);
    }
    for (int64_t i = tail0 + gid; i < n; i += nthreads) {
        mn = fminf(mn, (float)page[i]);
        mx = fmaxf(mx, (float)page[i]);
    }
    mn = wave_min(mn);
    mx = wave_max(mx);
    __shared__ float smn[4], smx[4];
    if ((threadIdx.x & 63) == 0) {
        smn[threadIdx.x >> 6] = mn;
        smx[threadIdx.x >> 6] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        mn = fminf(fminf(smn[0], smn[1]), fminf(smn[2], smn[3]));
        mx = fmaxf(fmaxf(smx[0], smx[1]), fmaxf(smx[2], smx[3]));
        // the words only grow, so a value already at or below one (however stale the read) changes
        // nothing: most workgroups skip their atomics, which would otherwise queue on two addresses
        const unsigned kmx = f32_ordered(mx), kmn = ~f32_ordered(mn);
        if (kmx > __atomic_load_n(ws + 0, __ATOMIC_RELAXED)) atomicMax(ws + 0, kmx);
        if (kmn > __atomic_load_n(ws + 1, __ATOMIC_RELAXED)) atomicMax(ws + 1, kmn);
        __threadfence();
        if (atomicAdd(ws + 2, 1u) == gridDim.x - 1) {        // the last workgroup: every other one's maxima are in
            __threadfence();
            out[0] = f32_unordered(~atomicMax(ws + 1, 0u));
            out[1] = f32_unordered(atomicMax(ws + 0, 0u));
        }
    }
}

// ---------------------------------------------------------------------- crops
constexpr int JOB_WORDS = 8;      // y0, x0, h, w, nw, Wb, offset / 32, box index (-1: top-up)
constexpr int RUN = 16;           // consecutive output columns of one row per thread: one 16-byte store
constexpr int TILE_COLS = 8 * RUN;

// (i, f) of destination index d of n over a source of s pixels (see the head of the file).
__device__ __forceinline__ void src_pos(int d, int s, int n, int& i, float& f) {
    const int num = (2 * d + 1) * s - n;
    i = 0;
    f = 0.0f;
    if (num > 0) {
        const unsigned q = (unsigned)num / (unsigned)(2 * n);
        if ((int)q >= s - 1) {
            i = s - 1;
        } else {
            i = (int)q;
            f = (float)(num - 2 * n * (int)q) / (float)(2 * n);
        }
    }
}

// grid (column tiles, jobs), 256 threads = 32 output rows x 8 runs of 16 columns.
template <typename T>
__global__ void __launch_bounds__(256) page_crops_kernel(const T* __restrict__ page, int H, int W,
                                                         const int4* __restrict__ jobs, uint8_t* __restrict__ arena,
                                                         const float* __restrict__ minmax, float scale) {
    const int4 ja = jobs[2 * blockIdx.y], jb = jobs[2 * blockIdx.y + 1];
    const int y0 = ja.x, x0 = ja.y, h = ja.z, w = ja.w, nw = jb.x, Wb = jb.y;
    const int row = threadIdx.x >> 3;
    const int col0 = blockIdx.x * TILE_COLS + (threadIdx.x & 7) * RUN;
    if (col0 >= Wb) return;
    unsigned px[RUN / 4] = {0u, 0u, 0u, 0u};
    if (col0 < nw) {
        float lo = 0.0f, gain = scale;
        if (minmax) {
            lo = minmax[0];
            const float range = minmax[1] - lo;
            gain = range > 0.0f ? scale / range : 0.0f;
        }
        int iy;
        float fy;
        src_pos(row, h, 32, iy, fy);
        // every source index is clamped into the page, whatever the table says
        const int ya = min(max(y0 + iy, 0), H - 1), yb = min(max(y0 + min(iy + 1, h - 1), 0), H - 1);
        const T* ra = page + (int64_t)ya * W;
        const T* rb = page + (int64_t)yb * W;
#pragma unroll
        for (int k = 0; k < RUN; ++k) {
            const int d = col0 + k;
            if (d < nw) {
                int ix;
                float fx;
                src_pos(d, w, nw, ix, fx);
                const int xa = min(max(x0 + ix, 0), W - 1), xb = min(max(x0 + min(ix + 1, w - 1), 0), W - 1);
                const float top = (float)ra[xa] * (1.0f - fx) + (float)ra[xb] * fx;
                const float bot = (float)rb[xa] * (1.0f - fx) + (float)rb[xb] * fx;
                const float v = top * (1.0f - fy) + bot * fy;
                const float q = fminf(fmaxf(floorf((v - lo) * gain), 0.0f), 255.0f);   // a NaN gives 0
                px[k >> 2] |= (unsigned)q << (8 * (k & 3));
            }
        }
    }
    uint8_t* dst = arena + (int64_t)jb.z * 32 + (int64_t)row * Wb + col0;
    *reinterpret_cast<uint4*>(dst) = make_uint4(px[0], px[1], px[2], px[3]);
}

}  // namespace

extern "C" int ocrk_page_minmax(const void* page, int dtype, int64_t n, float* minmax, void* ws, void* stream) {
    OCRK_REQUIRE(page && minmax && ws && n >= 1, "ocrk_page_minmax: bad arguments (n=%lld)", (long long)n);
    OCRK_REQUIRE(dtype == OCRK_F32 || dtype == OCRK_U8, "ocrk_page_minmax: a page is OCRK_F32 or OCRK_U8 (got %d)",
                 dtype);
    const uintptr_t addr = reinterpret_cast<uintptr_t>(page);
    const int esz = dtype == OCRK_F32 ? 4 : 1;
    OCRK_REQUIRE(addr % esz == 0 && (reinterpret_cast<uintptr_t>(minmax) & 3) == 0 &&
                     (reinterpret_cast<uintptr_t>(ws) & 3) == 0,
                 "ocrk_page_minmax: misaligned page, minmax or ws");
    int64_t head = (int64_t)((16 - addr % 16) % 16) / esz;
    if (head > n) head = n;
    hipStream_t s = ocrk::as_stream(stream);
    if (hipMemsetAsync(ws, 0, 16, s) != hipSuccess) return ocrk::launch_status("ocrk_page_minmax (memset)");
    const int64_t nvec = (n - head) / (16 / esz);
    const int64_t want = ocrk::cdiv(nvec > 0 ? nvec : 1, 256 * 4);      // ~4 vectors per thread before striding
    const int64_t cap = (int64_t)ocrk::cu_count() * 2;                  // every workgroup ends in same-address atomics
    dim3 grid((unsigned)(want < cap ? want : cap));
    if (dtype == OCRK_F32)
        page_minmax_kernel<float><<<grid, 256, 0, s>>>((const float*)page, n, (int)head, (unsigned*)ws, minmax);
    else
        page_minmax_kernel<uint8_t><<<grid, 256, 0, s>>>((const uint8_t*)page, n, (int)head, (unsigned*)ws, minmax);
    return ocrk::launch_status("ocrk_page_minmax");
}

extern "C" int ocrk_page_crops(const void* page, int dtype, int H, int W, const int* jobs, const int* jobs_host,
                               int njobs, uint8_t* arena, int64_t arena_bytes, const float* minmax, float scale,
                               void* stream) {
    OCRK_REQUIRE(njobs >= 0 && arena_bytes >= 0, "ocrk_page_crops: bad arguments (njobs=%d)", njobs);
    if (njobs == 0) return OCRK_OK;
    OCRK_REQUIRE(page && jobs && jobs_host && arena && H >= 1 && W >= 1,
                 "ocrk_page_crops: bad arguments (H=%d W=%d)", H, W);
    OCRK_REQUIRE(dtype == OCRK_F32 || dtype == OCRK_U8, "ocrk_page_crops: a page is OCRK_F32 or OCRK_U8 (got %d)",
                 dtype);
    OCRK_REQUIRE(scale == scale, "ocrk_page_crops: scale is NaN");
    OCRK_REQUIRE(reinterpret_cast<uintptr_t>(page) % (dtype == OCRK_F32 ? 4 : 1) == 0 &&
                     (reinterpret_cast<uintptr_t>(jobs) & 15) == 0 && (reinterpret_cast<uintptr_t>(arena) & 15) == 0 &&
                     (minmax == nullptr || (reinterpret_cast<uintptr_t>(minmax) & 3) == 0),
                 "ocrk_page_crops: misaligned page, jobs (16), arena (16) or minmax");
    OCRK_REQUIRE(njobs <= 65535, "ocrk_page_crops: at most 65535 jobs per launch (got %d)", njobs);
    int max_wb = 0;
    for (int j = 0; j < njobs; ++j) {
        const int* r = jobs_host + (int64_t)j * JOB_WORDS;
        const int64_t y0 = r[0], x0 = r[1], h = r[2], w = r[3], nw = r[4], wb = r[5], off = r[6];
        OCRK_REQUIRE(wb >= 32 && wb % 32 == 0 && wb <= (1 << 16), "ocrk_page_crops: job %d: Wb=%d is no multiple of 32",
                     j, (int)wb);
        OCRK_REQUIRE(off >= 0 && (off + wb) * 32 <= arena_bytes,
                     "ocrk_page_crops: job %d: bytes [%lld, %lld) lie outside the arena of %lld", j,
                     (long long)(off * 32), (long long)((off + wb) * 32), (long long)arena_bytes);
        if (r[7] < 0 && nw == 0) {          // a top-up crop: zeros, no source
            if (wb > max_wb) max_wb = (int)wb;
            continue;
        }
        OCRK_REQUIRE(nw >= 1 && nw <= wb, "ocrk_page_crops: job %d: nw=%d outside 1..Wb=%d", j, (int)nw, (int)wb);
        OCRK_REQUIRE(h >= 1 && w >= 1 && y0 >= 0 && x0 >= 0 && y0 + h <= H && x0 + w <= W,
                     "ocrk_page_crops: job %d: source rows [%d, %lld) x columns [%d, %lld) lie outside the %d x %d page",
                     j, (int)y0, (long long)(y0 + h), (int)x0, (long long)(x0 + w), H, W);
        OCRK_REQUIRE((2 * nw + 1) * w < (1ll << 31) && 63 * h < (1ll << 31),
                     "ocrk_page_crops: job %d: %d x %d -> width %d overflows the 32-bit sampling arithmetic", j, (int)h,
                     (int)w, (int)nw);
        if (wb > max_wb) max_wb = (int)wb;
    }
    dim3 grid((unsigned)ocrk::cdiv(max_wb, TILE_COLS), (unsigned)njobs);
    hipStream_t s = ocrk::as_stream(stream);
    if (dtype == OCRK_F32)
        page_crops_kernel<float><<<grid, 256, 0, s>>>((const float*)page, H, W, (const int4*)jobs, arena, minmax, scale);
    else
        page_crops_kernel<uint8_t><<<grid, 256, 0, s>>>((const uint8_t*)page, H, W, (const int4*)jobs, arena, minmax,
                                                       scale);
    return ocrk::launch_status("ocrk_page_crops");
}
