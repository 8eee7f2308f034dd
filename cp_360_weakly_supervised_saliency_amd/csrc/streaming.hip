// K24: viewport-adaptive streaming.  A viewer sees a window of the panorama, so a player fetches in high quality the tiles that
// are likely to be in somebody's window.  The model's map is a gaze density on hs x ws source pixels; source pixel j stands for a
// viewer whose head points at its centre, a level camera cam_j (utils/streaming.py: gaze_cameras, float64 on the host, rounded to
// f32 once).  The specification is the package's own, DESIGN.md "K24"; tests/streaming_restate.py restates it.
//
//   incidence   inc[j, i] = view_inside(cam_j, tx, ty, dir(i)) for the pixel i of the h x w grid - K17a's decision, bit for bit -
//               as bits: u32 [S, ceil(P / 32)], pixel i is bit i % 32 of word i / 32, the bits past P are 0.  It depends on the
//               two grids and the window only: computed once per planner, not per frame
//   tiles       rows x cols tiles on the grid, pixel (x, y) in tile ((y rows) / h) cols + (x cols) / w; tinc[j, t] = the OR of
//               inc[j, i] over the tile's pixels, in the same layout with P = T
//   expect      m[f, j] = sal[f, j] (float)a_y(row of j) if sal[f, j] > 0 and finite, else 0; for an output element i:
//               acc = 0, for j ascending: if bit(j, i): acc = acc + m[f, j], in f32; total[f] the same over every j;
//               out[f, i] = total > 0 ? acc / total : 0.  The one order is part of the definition
//   quality     for the viewer k of frame f and the levels u8 [F, T] of the tiles (a value >= L counts as L - 1):
//               qarea[k, l] = sum a_y [view_inside(R_k, dir(i)) and level(f, tile(i)) == l], exact integers
//
// Launches, on the caller's stream, no host synchronisation, no atomics:
//   K24a  incidence: grid (ceil(W32 / 256), S), a thread per (camera, word).  The 32 tests of a word stay in one lane, which
//         builds the word in a register and stores it: no cross-lane step between the decision and the store, neighbouring lanes
//         store neighbouring words, and the camera is the workgroup's (blockIdx.y), nine uniform values.  A wave per camera with
//         a ballot per 64 pixels would put the word into a scalar register pair first; it runs once per planner, so the
//         simpler form wins
//   K24b  tile incidence: grid (ceil(T32 / 64), S), a thread per (camera, word of 32 tiles); a tile's rows are bit ranges of inc
//   K24c  expect: grid (ceil(P / 256), ceil(F / 4)), a thread owns output element i of four frames; the masses of 256 source
//         pixels x 4 frames are staged in LDS (every lane reads the same address: a broadcast), the 32 lanes that share a word
//         read one address, the loop over j is sequential in every thread
//   K24d  quality: a wave per (viewer, frame) pair, four pairs per workgroup, as K17b: fix_frame, L int32 partial sums a lane
//         (at most 2^15 pixels of weight 1024), wave_sum_down in 64 bits, no LDS, no barrier.  The tile of a column and of a row
//         come from two int tables behind K11's in the workspace (an integer division per pixel costs as much as the decision)
#pragma clang fp contract(off)
#include "roc.h"

#include <math.h>

namespace {

constexpr int kIncThreads = 256;             // K24a
constexpr int kTincThreads = 64;             // K24b
constexpr int kExpThreads = 256;             // K24c: output elements per workgroup = source pixels staged at a time
constexpr int kExpFrames = 4;                // K24c: frames per thread
constexpr int kQualPairs = 4;                // K24d: pairs (waves) per workgroup
constexpr int kMaxLevels = 8;
constexpr int kMaxSource = 4096;             // S and T
constexpr int kMaxWeight = 1024;

// ------------------------------------------------------------------ K24a: incidence
// grid (ceil(W32 / 256), S), 256 threads
__global__ __launch_bounds__(kIncThreads) void view_incidence_kernel(const float* __restrict__ cams, const float2* __restrict__ tabx,
                                                                     const float2* __restrict__ taby, unsigned* __restrict__ inc,
                                                                     int h, int w, int W32, float tx, float ty) {
    const int word = blockIdx.x * kIncThreads + threadIdx.x;
    if (word >= W32) return;                                           // no barrier in this kernel
    const int j = blockIdx.y, P = h * w;
    const Rot cam = view_rot(cams + (size_t)j * 9);
    const int i0 = word * 32;
    int y = i0 / w, x = i0 - y * w;
    unsigned bits = 0;
#pragma unroll 4
    for (int b = 0; b < 32; ++b) {
        if (i0 + b < P) {
            float px, py, pz;
            stab_dir(tabx[x], taby[y], px, py, pz);
            bits |= (unsigned)view_inside(cam, tx, ty, px, py, pz) << b;
        }
        if (++x == w) {
            x = 0;
            ++y;
        }
    }
    inc[(size_t)j * W32 + word] = bits;
}

// ------------------------------------------------------------------ K24b: tile incidence
// the first pixel row (column) of tile row (column) t of n on an extent of e pixels: the least y with (y n) / e >= t
__device__ __forceinline__ int tile_first(int t, int n, int e) { return (int)(((long long)t * e + n - 1) / n); }

// whether any of the bits lo .. hi - 1 of a row of words is set
__device__ __forceinline__ bool any_bit(const unsigned* __restrict__ row, int lo, int hi) {
    const int w0 = lo >> 5, w1 = (hi - 1) >> 5;
    unsigned found = 0;
    for (int k = w0; k <= w1; ++k) {
        unsigned m = 0xffffffffu;
        if (k == w0) m &= 0xffffffffu << (lo & 31);
        if (k == w1) m &= 0xffffffffu >> (31 - ((hi - 1) & 31));
        found |= row[k] & m;
    }
    return found != 0;
}

// grid (ceil(T32 / 64), S), 64 threads
__global__ __launch_bounds__(kTincThreads) void tile_incidence_kernel(const unsigned* __restrict__ inc, unsigned* __restrict__ tinc,
                                                                      int h, int w, int rows, int cols, int W32, int T32) {
    const int word = blockIdx.x * kTincThreads + threadIdx.x;
    if (word >= T32) return;
    const int j = blockIdx.y, T = rows * cols;
    const unsigned* row = inc + (size_t)j * W32;
    unsigned bits = 0;
    for (int b = 0; b < 32; ++b) {
        const int t = word * 32 + b;
        if (t >= T) break;
        const int tr = t / cols, tc = t - tr * cols;
        const int y0 = tile_first(tr, rows, h), y1 = tile_first(tr + 1, rows, h);
        const int x0 = tile_first(tc, cols, w), x1 = tile_first(tc + 1, cols, w);
        bool any = false;
        for (int y = y0; y < y1 && !any; ++y) any = any_bit(row, y * w + x0, y * w + x1);
        bits |= (unsigned)any << b;
    }
    tinc[(size_t)j * T32 + word] = bits;
}

// ------------------------------------------------------------------ K24c: expectation
__device__ __forceinline__ float view_mass(float s, int a) { return s > 0.f && isfinite(s) ? s * (float)a : 0.f; }

// grid (ceil(P / 256), ceil(F / 4)), 256 threads
__global__ __launch_bounds__(kExpThreads) void view_expect_kernel(const float* __restrict__ sal, const int* __restrict__ weights,
                                                                  const unsigned* __restrict__ bits, float* __restrict__ out,
                                                                  float* __restrict__ total, int F, int S, int ws, int P, int W32) {
    __shared__ float4 mass[kExpThreads];                               // [source pixel of the chunk] x (four frames)
    static_assert(kExpFrames == 4, "a float4 of masses per source pixel");
    const int tid = threadIdx.x, f0 = blockIdx.y * kExpFrames;
    const int i = blockIdx.x * kExpThreads + tid;
    const int iw = i < P ? i >> 5 : 0, ib = i & 31;                    // a thread past P keeps the barriers' company and stores nothing
    float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f, acc3 = 0.f, tot0 = 0.f, tot1 = 0.f, tot2 = 0.f, tot3 = 0.f;
    for (int j0 = 0; j0 < S; j0 += kExpThreads) {                      // S is the workgroup's: the barriers are uniform
        const int j = j0 + tid;
        if (j < S) {
            const int a = fix_clamp(weights[j / ws], 0, kMaxWeight);
            float4 m;
            m.x = view_mass(sal[(size_t)f0 * S + j], a);
            m.y = f0 + 1 < F ? view_mass(sal[(size_t)(f0 + 1) * S + j], a) : 0.f;
            m.z = f0 + 2 < F ? view_mass(sal[(size_t)(f0 + 2) * S + j], a) : 0.f;
            m.w = f0 + 3 < F ? view_mass(sal[(size_t)(f0 + 3) * S + j], a) : 0.f;
            mass[tid] = m;
        }
        __syncthreads();
        const int n = S - j0 < kExpThreads ? S - j0 : kExpThreads;
        const unsigned* col = bits + (size_t)j0 * W32 + iw;
        for (int c = 0; c < n; ++c) {
            const bool in = (col[(size_t)c * W32] >> ib) & 1u;
            const float4 m = mass[c];
            acc0 = in ? acc0 + m.x : acc0;
            acc1 = in ? acc1 + m.y : acc1;
            acc2 = in ? acc2 + m.z : acc2;
            acc3 = in ? acc3 + m.w : acc3;
            tot0 = tot0 + m.x;
            tot1 = tot1 + m.y;
            tot2 = tot2 + m.z;
            tot3 = tot3 + m.w;
        }
        __syncthreads();
    }
    const float acc[kExpFrames] = {acc0, acc1, acc2, acc3}, tot[kExpFrames] = {tot0, tot1, tot2, tot3};
#pragma unroll
    for (int k = 0; k < kExpFrames; ++k) {
        if (f0 + k >= F) break;
        if (i < P) out[(size_t)(f0 + k) * P + i] = tot[k] > 0.f ? acc[k] / tot[k] : 0.f;
        if (blockIdx.x == 0 && tid == 0) total[f0 + k] = tot[k];
    }
}

// ------------------------------------------------------------------ K24d: delivered quality
// tcol int [w] = (x cols) / w, trow int [h] = ((y rows) / h) cols: tile(x, y) = trow[y] + tcol[x]
__global__ __launch_bounds__(256) void tile_tables_kernel(int* __restrict__ tcol, int* __restrict__ trow, int h, int w, int rows,
                                                          int cols) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < w) tcol[i] = (int)(((long long)i * cols) / w);
    else if (i < w + h) trow[i - w] = (int)(((long long)(i - w) * rows) / h) * cols;
}

// grid ceil(N / 4), 256 threads; the frame of pair k is sphere.h's fix_frame
__global__ __launch_bounds__(64 * kQualPairs) void view_quality_kernel(const float* __restrict__ R, const int* __restrict__ offsets, int N,
                                                                       int F, const float2* __restrict__ tabx,
                                                                       const float2* __restrict__ taby, const int* __restrict__ tcol,
                                                                       const int* __restrict__ trow, const int* __restrict__ weights,
                                                                       const unsigned char* __restrict__ levels, long long* __restrict__ qarea,
                                                                       int h, int w, int T, int L, float tx, float ty) {
    const int lane = threadIdx.x & 63;
    const long long k = (long long)blockIdx.x * kQualPairs + (threadIdx.x >> 6);
    if (k >= N) return;                                                // the whole wave; the kernel has no barrier
    const unsigned char* lev = levels + (size_t)fix_frame(offsets, F, (int)k) * T;
    const Rot view = view_rot(R + k * 9);
    const int P = h * w;
    int x = lane % w, y = lane / w;
    int s[kMaxLevels] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = lane; i < P; i += 64) {
        float px, py, pz;
        stab_dir(tabx[x], taby[y], px, py, pz);
        const bool v = view_inside(view, tx, ty, px, py, pz);
        const int a = v ? fix_clamp(weights[y], 0, kMaxWeight) : 0;
        int l = lev[trow[y] + tcol[x]];
        l = l < L ? l : L - 1;
#pragma unroll
        for (int q = 0; q < kMaxLevels; ++q) s[q] += l == q ? a : 0;
        x += 64;
        while (x >= w) {
            x -= w;
            ++y;
        }
    }
#pragma unroll
    for (int q = 0; q < kMaxLevels; ++q) {
        if (q >= L) break;                                             // L is the launch's: uniform
        const long long t = wave_sum_down((long long)s[q]);
        if (lane == 0) qarea[k * L + q] = t;
    }
}

// ------------------------------------------------------------------ host side
// rows x cols tiles on an h x w grid
int tile_args(int h, int w, int rows, int cols) {
    if (h < 1 || w < 1 || rows < 1 || cols < 1 || rows > h || cols > w) return CP360_ERR_BAD_SHAPE;
    if ((long long)h * w > kRocMaxP || (long long)rows * cols > kMaxSource) return CP360_ERR_UNSUPPORTED;
    return CP360_OK;
}

size_t quality_bytes(int h, int w) { return tab_bytes(h, w) + align16((size_t)w * sizeof(int)) + align16((size_t)h * sizeof(int)); }

}  // namespace

// ------------------------------------------------------------------ C ABI
extern "C" int cp360_view_incidence(const float* cams, int S, int h, int w, double hfov_rad, double aspect, uint32_t* inc, void* work,
                                    size_t work_bytes, void* stream) {
    if (!cams || !inc || !work) return CP360_ERR_NULL;
    float tx, ty;
    if (S < 1 || h < 1 || w < 1 || !head_tangents(hfov_rad, aspect, &tx, &ty)) return CP360_ERR_BAD_SHAPE;
    if (S > kMaxSource || (long long)h * w > kRocMaxP) return CP360_ERR_UNSUPPORTED;
    if ((((uintptr_t)cams | (uintptr_t)inc) & 3) != 0) return CP360_ERR_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    SphereTabs t;
    const int st = open_tabs(work, work_bytes, tab_bytes(h, w), h, w, s, &t);
    if (st != CP360_OK) return st;
    const int W32 = (h * w + 31) / 32;
    hipLaunchKernelGGL(view_incidence_kernel, dim3((W32 + kIncThreads - 1) / kIncThreads, S), dim3(kIncThreads), 0, s, cams, t.x, t.y,
                       (unsigned*)inc, h, w, W32, tx, ty);
    CP360_CHECK_HIP();
    return CP360_OK;
}

extern "C" int cp360_tile_incidence(const uint32_t* inc, int S, int h, int w, int rows, int cols, uint32_t* tinc, void* stream) {
    if (!inc || !tinc) return CP360_ERR_NULL;
    if (S < 1) return CP360_ERR_BAD_SHAPE;
    const int st = tile_args(h, w, rows, cols);
    if (st != CP360_OK) return st;
    if (S > kMaxSource) return CP360_ERR_UNSUPPORTED;
    if ((((uintptr_t)inc | (uintptr_t)tinc) & 3) != 0) return CP360_ERR_ALIGN;
    const int W32 = (h * w + 31) / 32, T32 = (rows * cols + 31) / 32;
    hipLaunchKernelGGL(tile_incidence_kernel, dim3((T32 + kTincThreads - 1) / kTincThreads, S), dim3(kTincThreads), 0, (hipStream_t)stream,
                       (const unsigned*)inc, (unsigned*)tinc, h, w, rows, cols, W32, T32);
    CP360_CHECK_HIP();
    return CP360_OK;
}

extern "C" int cp360_view_expect(const float* sal, int F, int hs, int ws, const int32_t* weights, const uint32_t* bits, int P, float* out,
                                 float* total, void* stream) {
    if (!weights || !bits || ((!sal || !out || !total) && F > 0)) return CP360_ERR_NULL;
    if (F < 0 || hs < 1 || ws < 1 || P < 1) return CP360_ERR_BAD_SHAPE;
    if (F > 65535 || (long long)hs * ws > kMaxSource || P > kRocMaxP) return CP360_ERR_UNSUPPORTED;
    if ((((uintptr_t)sal | (uintptr_t)weights | (uintptr_t)bits | (uintptr_t)out | (uintptr_t)total) & 3) != 0) return CP360_ERR_ALIGN;
    if (F == 0) return CP360_OK;                                       // no frames: nothing to launch
    hipLaunchKernelGGL(view_expect_kernel, dim3((P + kExpThreads - 1) / kExpThreads, (F + kExpFrames - 1) / kExpFrames), dim3(kExpThreads),
                       0, (hipStream_t)stream, sal, (const int*)weights, (const unsigned*)bits, out, total, F, hs * ws, ws, P,
                       (P + 31) / 32);
    CP360_CHECK_HIP();
    return CP360_OK;
}

extern "C" size_t cp360_view_quality_work_bytes(int h, int w) {
    if (h < 1 || w < 1 || (long long)h * w > kRocMaxP) return 0;
    return quality_bytes(h, w);
}

extern "C" int cp360_view_quality(const float* R, const int32_t* offsets, long long N, int F, int h, int w, double hfov_rad, double aspect,
                                  const int32_t* weights, const uint8_t* levels, int rows, int cols, int L, long long* qarea, void* work,
                                  size_t work_bytes, void* stream) {
    if (!offsets || !weights || !work || ((!R || !levels || !qarea) && N > 0)) return CP360_ERR_NULL;
    float tx, ty;
    if (F < 0 || N < 0 || (F == 0 && N > 0) || L < 1 || L > kMaxLevels || !head_tangents(hfov_rad, aspect, &tx, &ty))
        return CP360_ERR_BAD_SHAPE;
    int st = tile_args(h, w, rows, cols);
    if (st != CP360_OK) return st;
    if (F > 65535 || N >= (1LL << 31)) return CP360_ERR_UNSUPPORTED;
    if ((((uintptr_t)R | (uintptr_t)offsets | (uintptr_t)weights) & 3) != 0 || ((uintptr_t)qarea & 7) != 0) return CP360_ERR_ALIGN;
    st = check_work(work, work_bytes, quality_bytes(h, w));
    if (st != CP360_OK || N == 0) return st;                           // no pairs: nothing to launch
    hipStream_t s = (hipStream_t)stream;
    SphereTabs t;
    st = launch_tables(work, h, w, s, &t);
    if (st != CP360_OK) return st;
    int* tcol = (int*)((char*)work + tab_bytes(h, w));
    int* trow = (int*)((char*)tcol + align16((size_t)w * sizeof(int)));
    hipLaunchKernelGGL(tile_tables_kernel, dim3((h + w + 255) / 256), dim3(256), 0, s, tcol, trow, h, w, rows, cols);
    CP360_CHECK_HIP();
    hipLaunchKernelGGL(view_quality_kernel, dim3((unsigned)((N + kQualPairs - 1) / kQualPairs)), dim3(64 * kQualPairs), 0, s, R,
                       (const int*)offsets, (int)N, F, t.x, t.y, (const int*)tcol, (const int*)trow, (const int*)weights, levels, qarea, h,
                       w, rows * cols, L, tx, ty);
    CP360_CHECK_HIP();
    return CP360_OK;
}
