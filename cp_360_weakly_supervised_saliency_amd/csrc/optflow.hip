// K10: dense optical flow after Farneback (utils/optical_flow.py:32 of the reference, the cv2.calcOpticalFlowFarneback line
// beneath its DeepFlow call), batched over the frames of a video.  The package's definition is DESIGN.md "K10"; in short:
//
//   gray      u8 RGB frame (already resized) -> (c0 1868 + c1 9617 + c2 4899 + 8192) >> 14 on the REVERSED channels, as f32
//   pyramid   level k = bilinear resize (half-pixel centres, edge clamp) of the ksz x ksz Gaussian blur (reflect-101) of the
//             full-resolution gray image; scale = pyr_scale^k, sigma = (1 / scale - 1) / 2, ksz = max(cvRound(5 sigma) | 1, 3)
//   expand    separable (2n+1)^2 polynomial expansion, replicate-clamped: R = coefficients of [y, x, y^2, x^2, xy]
//   matrices  R of prev at the pixel, R of next sampled bilinearly at pixel + flow -> the five sums M of the 2 x 2 system
//   solve     (2m+1)^2 box mean of M, replicate-clamped, then the 2 x 2 solve with + 1e-3 on the determinant
//   upsample  bilinear resize of the flow to the next finer level times 1 / pyr_scale
//
// Layouts: images f32 [N, h, w]; R f32 [N, 5, h, w] and M f32 [P, 5, h, w] are PLANAR (the matrices kernel gathers 4
// neighbours x 5 channels at a data-dependent position: in planes the lanes of a wave read neighbouring addresses); flow f32
// [P, h, w, 2] = (dx, dy), the layout of the reference's motion/*.npy.  Every frame's pyramid level and expansion is computed
// once: pair p reads R[p] and R[p + 1].
//
// The expansion and the box sums are separable passes inside one workgroup over a 64 x 16 tile staged with its halo (n, m) in
// LDS; each thread finishes 4 neighbouring pixels of one row and stores them as 16-byte pieces when the row length is a
// multiple of 4.  No atomics, every sum in a fixed order: results are bit-reproducible and do not depend on the batch size.
#include "common.h"
#include "../../include/cp360.h"

#include <math.h>

namespace {

constexpr int kMaxPolyN = 7;                 // poly_n <= 7: 15 taps
constexpr int kMaxBoxM = 16;                 // winsize <= 33
constexpr int kMaxKsz = 255;                 // Gaussian of a pyramid level
constexpr int kMaxLevels = 32;               // coarser levels the driver handles
constexpr int kTW = 64, kTH = 16;            // output tile of the two stencil kernels (256 threads x 4 pixels)
constexpr int kPitchE = kTW + 2 * kMaxPolyN; // LDS row pitch of the expansion
constexpr int kPitchB = kTW + 2 * kMaxBoxM;  // LDS row pitch of the box sums

struct GaussTaps {
    float v[kMaxKsz + 1];
};
struct PolyTabs {
    float g[2 * kMaxPolyN + 1], xg[2 * kMaxPolyN + 1], xxg[2 * kMaxPolyN + 1];
    float ig11, ig03, ig33, ig55;
};

// reflect-101 (gfedcb|abcdefgh|gfedcba) folded as often as it takes: the period is 2 (n - 1); n = 1 has one pixel.
__host__ __device__ __forceinline__ int reflect101(int i, int n) {
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - i;
}

// One axis of the bilinear resize (half-pixel centres, edge clamp): the arithmetic of cp360_resize_linear_f32.
__device__ __forceinline__ void lin_tap(int d, int n_src, int n_dst, int& i0, int& i1, float& fr) {
    const double scale = (double)n_src / (double)n_dst;
    const double f = ((double)d + 0.5) * scale - 0.5;
    int i = (int)floor(f);
    float t = (float)(f - (double)i);
    if (i < 0) { i = 0; t = 0.f; }
    if (i >= n_src - 1) { i = n_src - 1; t = 0.f; }
    i0 = i;
    i1 = min(i + 1, n_src - 1);
    fr = t;
}

// ------------------------------------------------------------------ gray
__global__ __launch_bounds__(256) void gray_kernel(const uint8_t* __restrict__ rgb, float* __restrict__ gray, long long n) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const uint8_t* p = rgb + 3 * i;
        // channels reversed first: c0 = p[2], c1 = p[1], c2 = p[0]
        gray[i] = (float)(((int)p[2] * 1868 + (int)p[1] * 9617 + (int)p[0] * 4899 + 8192) >> 14);
    }
}

// ------------------------------------------------------------------ pyramid level
// horizontal Gaussian at full resolution: grid (ceil(W / 256), H, N)
__global__ __launch_bounds__(256) void pyr_hblur_kernel(const float* __restrict__ src, float* __restrict__ dst, int H, int W,
                                                        int ksz, GaussTaps taps) {
    __shared__ float sk[kMaxKsz + 1];
    if ((int)threadIdx.x < ksz) sk[threadIdx.x] = taps.v[threadIdx.x];
    __syncthreads();
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= W) return;
    const size_t row_off = ((size_t)blockIdx.z * H + blockIdx.y) * W;
    const float* row = src + row_off;
    const int r = ksz >> 1;
    float acc = 0.f;
    for (int k = 0; k < ksz; ++k) acc += sk[k] * row[reflect101(x + k - r, W)];
    dst[row_off + x] = acc;
}

// vertical Gaussian of the four rows-by-columns the bilinear tap needs, then the tap: grid (ceil(lw / 256), lh, N)
__global__ __launch_bounds__(256) void pyr_vresize_kernel(const float* __restrict__ tmp, float* __restrict__ dst, int H, int W,
                                                          int lh, int lw, int ksz, GaussTaps taps) {
    __shared__ float sk[kMaxKsz + 1];
    if ((int)threadIdx.x < ksz) sk[threadIdx.x] = taps.v[threadIdx.x];
    __syncthreads();
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= lw) return;
    int y0, y1, x0, x1;
    float fy, fx;
    lin_tap(y, H, lh, y0, y1, fy);
    lin_tap(x, W, lw, x0, x1, fx);
    const float* img = tmp + (size_t)blockIdx.z * H * W;
    const int r = ksz >> 1;
    float a = 0.f, b = 0.f, c = 0.f, d = 0.f;
    for (int k = 0; k < ksz; ++k) {
        const float* r0 = img + (size_t)reflect101(y0 + k - r, H) * W;
        const float* r1 = img + (size_t)reflect101(y1 + k - r, H) * W;
        const float g = sk[k];
        a += g * r0[x0];
        b += g * r0[x1];
        c += g * r1[x0];
        d += g * r1[x1];
    }
    const float top = a * (1.f - fx) + b * fx;
    const float bot = c * (1.f - fx) + d * fx;
    dst[((size_t)blockIdx.z * lh + y) * lw + x] = top * (1.f - fy) + bot * fy;
}

// ------------------------------------------------------------------ flow to the next finer level
__global__ __launch_bounds__(256) void flow_upsample_kernel(const float2* __restrict__ in, int h, int w, float2* __restrict__ out,
                                                            int nh, int nw, float mul) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= nw) return;
    int y0, y1, x0, x1;
    float fy, fx;
    lin_tap(y, h, nh, y0, y1, fy);
    lin_tap(x, w, nw, x0, x1, fx);
    const float2* img = in + (size_t)blockIdx.z * h * w;
    const float2 a = img[(size_t)y0 * w + x0], b = img[(size_t)y0 * w + x1];
    const float2 c = img[(size_t)y1 * w + x0], d = img[(size_t)y1 * w + x1];
    const float tx = a.x * (1.f - fx) + b.x * fx, bx = c.x * (1.f - fx) + d.x * fx;
    const float ty = a.y * (1.f - fx) + b.y * fx, by = c.y * (1.f - fx) + d.y * fx;
    out[((size_t)blockIdx.z * nh + y) * nw + x] = make_float2((tx * (1.f - fy) + bx * fy) * mul, (ty * (1.f - fy) + by * fy) * mul);
}

// ------------------------------------------------------------------ polynomial expansion
// grid (ceil(w / 64), ceil(h / 16), N).  Thread t finishes pixels x = 4 (t % 16) .. + 3 of tile row t / 16.
__global__ __launch_bounds__(256) void poly_exp_kernel(const float* __restrict__ img, float* __restrict__ R, int h, int w, int n,
                                                       int vec, PolyTabs tabs) {
    __shared__ float s_in[(kTH + 2 * kMaxPolyN) * kPitchE];
    __shared__ float s_r[3][kTH * kPitchE];
    __shared__ float s_g[3][2 * kMaxPolyN + 2];
    const int tid = threadIdx.x, taps = 2 * n + 1;
    if (tid < taps) {
        s_g[0][tid] = tabs.g[tid];
        s_g[1][tid] = tabs.xg[tid];
        s_g[2][tid] = tabs.xxg[tid];
    }
    const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
    const size_t hw = (size_t)h * w;
    const float* src = img + (size_t)blockIdx.z * hw;
    const int cols = kTW + 2 * n, rows = kTH + 2 * n;
    for (int i = tid; i < rows * cols; i += 256) {
        const int ry = i / cols, rx = i - ry * cols;
        const int gy = min(max(y0 + ry - n, 0), h - 1), gx = min(max(x0 + rx - n, 0), w - 1);
        s_in[ry * kPitchE + rx] = src[(size_t)gy * w + gx];
    }
    __syncthreads();
    for (int i = tid; i < kTH * cols; i += 256) {                 // vertical pass: r0, r1, r2 of every staged column
        const int ry = i / cols, rx = i - ry * cols;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
        for (int k = 0; k < taps; ++k) {
            const float v = s_in[(ry + k) * kPitchE + rx];
            a0 += s_g[0][k] * v;
            a1 += s_g[1][k] * v;
            a2 += s_g[2][k] * v;
        }
        s_r[0][ry * kPitchE + rx] = a0;
        s_r[1][ry * kPitchE + rx] = a1;
        s_r[2][ry * kPitchE + rx] = a2;
    }
    __syncthreads();
    const int ty = tid >> 4, tx = (tid & 15) * 4;
    float b1[4] = {0.f, 0.f, 0.f, 0.f}, b2[4] = {0.f, 0.f, 0.f, 0.f}, b3[4] = {0.f, 0.f, 0.f, 0.f};
    float b4[4] = {0.f, 0.f, 0.f, 0.f}, b5[4] = {0.f, 0.f, 0.f, 0.f}, b6[4] = {0.f, 0.f, 0.f, 0.f};
    const int base = ty * kPitchE + tx;
    for (int j = 0; j < taps + 3; ++j) {                          // horizontal pass: column j of the window feeds <= 4 pixels
        const float r0 = s_r[0][base + j], r1 = s_r[1][base + j], r2 = s_r[2][base + j];
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const int k = j - o;
            if (k >= 0 && k < taps) {
                const float g = s_g[0][k], xg = s_g[1][k], xxg = s_g[2][k];
                b1[o] += g * r0;
                b2[o] += xg * r0;
                b3[o] += g * r1;
                b4[o] += xxg * r0;
                b5[o] += g * r2;
                b6[o] += xg * r1;
            }
        }
    }
    const int y = y0 + ty, x = x0 + tx;
    if (y >= h || x >= w) return;
    float o0[4], o1[4], o2[4], o3[4], o4[4];
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        o0[o] = b3[o] * tabs.ig11;
        o1[o] = b2[o] * tabs.ig11;
        o2[o] = b1[o] * tabs.ig03 + b5[o] * tabs.ig33;
        o3[o] = b1[o] * tabs.ig03 + b4[o] * tabs.ig33;
        o4[o] = b6[o] * tabs.ig55;
    }
    float* dst = R + (size_t)blockIdx.z * 5 * hw + (size_t)y * w + x;
    if (vec) {                                                    // w % 4 == 0: x + 3 < w, 16-byte aligned
        *(float4*)(dst) = make_float4(o0[0], o0[1], o0[2], o0[3]);
        *(float4*)(dst + hw) = make_float4(o1[0], o1[1], o1[2], o1[3]);
        *(float4*)(dst + 2 * hw) = make_float4(o2[0], o2[1], o2[2], o2[3]);
        *(float4*)(dst + 3 * hw) = make_float4(o3[0], o3[1], o3[2], o3[3]);
        *(float4*)(dst + 4 * hw) = make_float4(o4[0], o4[1], o4[2], o4[3]);
    } else {
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            if (x + o < w) {
                dst[o] = o0[o];
                dst[hw + o] = o1[o];
                dst[2 * hw + o] = o2[o];
                dst[3 * hw + o] = o3[o];
                dst[4 * hw + o] = o4[o];
            }
        }
    }
}

// ------------------------------------------------------------------ matrices
__device__ __forceinline__ float edge_factor(int d) { return d < 2 ? 0.14f : (d < 5 ? 0.4472f : 1.f); }

// grid (ceil(h w / 256), P): one pixel per thread; pair p reads R0 + p r_stride (prev) and R1 + p r_stride (next)
__global__ __launch_bounds__(256) void matrices_kernel(const float* __restrict__ R0, const float* __restrict__ R1, size_t r_stride,
                                                       const float2* __restrict__ flow, float* __restrict__ M, int h, int w) {
    const int hw = h * w;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= hw) return;
    const int p = blockIdx.y;
    const int y = idx / w, x = idx - y * w;
    const float* r0 = R0 + (size_t)p * r_stride + idx;
    const float* r1 = R1 + (size_t)p * r_stride;
    const float2 d = flow[(size_t)p * hw + idx];
    const float dx = d.x, dy = d.y;
    const float fx = (float)x + dx, fy = (float)y + dy;
    const float x1f = floorf(fx), y1f = floorf(fy);
    const float a0 = r0[0], a1 = r0[hw], a2 = r0[2 * (size_t)hw], a3 = r0[3 * (size_t)hw], a4 = r0[4 * (size_t)hw];
    float r2, r3, r4, r5, r6;
    // compared as floats, so a NaN or huge flow takes the outside branch and never becomes an index
    if (x1f >= 0.f && x1f < (float)(w - 1) && y1f >= 0.f && y1f < (float)(h - 1)) {
        const float ax = fx - x1f, ay = fy - y1f;
        const float w00 = (1.f - ax) * (1.f - ay), w01 = ax * (1.f - ay), w10 = (1.f - ax) * ay, w11 = ax * ay;
        const float* q = r1 + (size_t)(int)y1f * w + (int)x1f;
        float s[5];
#pragma unroll
        for (int c = 0; c < 5; ++c) {
            const float* qc = q + (size_t)c * hw;
            s[c] = w00 * qc[0] + w01 * qc[1] + w10 * qc[w] + w11 * qc[w + 1];
        }
        r2 = s[0];
        r3 = s[1];
        r4 = (a2 + s[2]) * 0.5f;
        r5 = (a3 + s[3]) * 0.5f;
        r6 = (a4 + s[4]) * 0.25f;
    } else {
        r2 = r3 = 0.f;
        r4 = a2;
        r5 = a3;
        r6 = a4 * 0.5f;
    }
    r2 = (a0 - r2) * 0.5f;
    r3 = (a1 - r3) * 0.5f;
    r2 += r4 * dy + r6 * dx;
    r3 += r6 * dy + r5 * dx;
    const float sc = edge_factor(x) * edge_factor(w - 1 - x) * edge_factor(y) * edge_factor(h - 1 - y);
    r2 *= sc;
    r3 *= sc;
    r4 *= sc;
    r5 *= sc;
    r6 *= sc;
    float* m = M + (size_t)p * 5 * hw + idx;
    m[0] = r4 * r4 + r6 * r6;
    m[hw] = (r4 + r5) * r6;
    m[2 * (size_t)hw] = r5 * r5 + r6 * r6;
    m[3 * (size_t)hw] = r4 * r2 + r6 * r3;
    m[4 * (size_t)hw] = r6 * r2 + r5 * r3;
}

// ------------------------------------------------------------------ box mean and 2 x 2 solve
// The (2m+1)^2 box SUM of one plane for the thread's 4 pixels; s_t / s_v are the workgroup's staging tile and column sums.
__device__ __forceinline__ void box4(const float* __restrict__ plane, int h, int w, int m, int x0, int y0, float* s_t, float* s_v,
                                     float (&out)[4]) {
    const int tid = threadIdx.x;
    const int cols = kTW + 2 * m, rows = kTH + 2 * m, taps = 2 * m + 1;
    __syncthreads();                                               // the previous plane's sums have been read
    for (int i = tid; i < rows * cols; i += 256) {
        const int ry = i / cols, rx = i - ry * cols;
        const int gy = min(max(y0 + ry - m, 0), h - 1), gx = min(max(x0 + rx - m, 0), w - 1);
        s_t[ry * kPitchB + rx] = plane[(size_t)gy * w + gx];
    }
    __syncthreads();
    for (int i = tid; i < kTH * cols; i += 256) {                 // column sums of every staged column
        const int ry = i / cols, rx = i - ry * cols;
        float s = 0.f;
        for (int k = 0; k < taps; ++k) s += s_t[(ry + k) * kPitchB + rx];
        s_v[ry * kPitchB + rx] = s;
    }
    __syncthreads();
    const int base = (tid >> 4) * kPitchB + (tid & 15) * 4;
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < taps + 3; ++j) {
        const float v = s_v[base + j];
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const int k = j - o;
            if (k >= 0 && k < taps) a[o] += v;
        }
    }
#pragma unroll
    for (int o = 0; o < 4; ++o) out[o] = a[o];
}

// grid (ceil(w / 64), ceil(h / 16), P)
__global__ __launch_bounds__(256) void blur_solve_kernel(const float* __restrict__ M, float* __restrict__ flow, int h, int w, int m,
                                                         float inv_area, int vec) {
    __shared__ float s_t[(kTH + 2 * kMaxBoxM) * kPitchB];
    __shared__ float s_v[kTH * kPitchB];
    const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
    const size_t hw = (size_t)h * w;
    const float* Mp = M + (size_t)blockIdx.z * 5 * hw;
    float g11[4], g12[4], g22[4], h1[4], h2[4];
    box4(Mp, h, w, m, x0, y0, s_t, s_v, g11);
    box4(Mp + hw, h, w, m, x0, y0, s_t, s_v, g12);
    box4(Mp + 2 * hw, h, w, m, x0, y0, s_t, s_v, g22);
    box4(Mp + 3 * hw, h, w, m, x0, y0, s_t, s_v, h1);
    box4(Mp + 4 * hw, h, w, m, x0, y0, s_t, s_v, h2);
    const int y = y0 + (threadIdx.x >> 4), x = x0 + (threadIdx.x & 15) * 4;
    if (y >= h || x >= w) return;
    float fx[4], fy[4];
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const float a = g11[o] * inv_area, b = g12[o] * inv_area, c = g22[o] * inv_area;
        const float p = h1[o] * inv_area, q = h2[o] * inv_area;
        const float idet = 1.f / (a * c - b * b + 1e-3f);
        fx[o] = (a * q - b * p) * idet;
        fy[o] = (c * p - b * q) * idet;
    }
    float* dst = flow + ((size_t)blockIdx.z * hw + (size_t)y * w + x) * 2;
    if (vec) {
        *(float4*)(dst) = make_float4(fx[0], fy[0], fx[1], fy[1]);
        *(float4*)(dst + 4) = make_float4(fx[2], fy[2], fx[3], fy[3]);
    } else {
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            if (x + o < w) {
                dst[2 * o] = fx[o];
                dst[2 * o + 1] = fy[o];
            }
        }
    }
}

// ------------------------------------------------------------------ host side
int cv_round(double v) { return (int)nearbyint(v); }              // round half to even (the default rounding mode)

int gauss_taps(int ksz, double sigma, GaussTaps* t) {
    if (ksz < 1 || ksz > kMaxKsz || !(ksz & 1)) return CP360_ERR_UNSUPPORTED;
    for (int i = 0; i <= kMaxKsz; ++i) t->v[i] = 0.f;
    return cp360_optflow_gauss_host(ksz, sigma, t->v);
}

int poly_tabs(int n, double sigma, PolyTabs* t) {
    float ig[4];
    const int st = cp360_optflow_poly_tables_host(n, sigma, t->g, t->xg, t->xxg, ig);
    if (st != CP360_OK) return st;
    for (int i = 2 * n + 1; i < 2 * kMaxPolyN + 1; ++i) t->g[i] = t->xg[i] = t->xxg[i] = 0.f;
    t->ig11 = ig[0];
    t->ig03 = ig[1];
    t->ig33 = ig[2];
    t->ig55 = ig[3];
    return CP360_OK;
}

int launch_pyr_level(const float* gray, int N, int H, int W, const GaussTaps& taps, int ksz, float* out, int lh, int lw,
                     float* tmp, hipStream_t s) {
    hipLaunchKernelGGL(pyr_hblur_kernel, dim3((W + 255) / 256, H, N), dim3(256), 0, s, gray, tmp, H, W, ksz, taps);
    CP360_CHECK_HIP();
    hipLaunchKernelGGL(pyr_vresize_kernel, dim3((lw + 255) / 256, lh, N), dim3(256), 0, s, (const float*)tmp, out, H, W, lh, lw,
                       ksz, taps);
    CP360_CHECK_HIP();
    return CP360_OK;
}

int launch_poly_exp(const float* img, int N, int h, int w, int n, const PolyTabs& tabs, float* R, hipStream_t s) {
    const int vec = (w % 4 == 0) && aligned16(R);
    hipLaunchKernelGGL(poly_exp_kernel, dim3((w + kTW - 1) / kTW, (h + kTH - 1) / kTH, N), dim3(256), 0, s, img, R, h, w, n, vec,
                       tabs);
    CP360_CHECK_HIP();
    return CP360_OK;
}

int launch_matrices(const float* R0, const float* R1, size_t r_stride, const float* flow, float* M, int P, int h, int w,
                    hipStream_t s) {
    hipLaunchKernelGGL(matrices_kernel, dim3((h * w + 255) / 256, P), dim3(256), 0, s, R0, R1, r_stride, (const float2*)flow, M, h,
                       w);
    CP360_CHECK_HIP();
    return CP360_OK;
}

int launch_blur_solve(const float* M, float* flow, int P, int h, int w, int winsize, hipStream_t s) {
    const int m = winsize / 2;
    const int vec = (w % 4 == 0) && aligned16(flow);
    const float inv_area = (float)(1.0 / ((double)(2 * m + 1) * (2 * m + 1)));
    hipLaunchKernelGGL(blur_solve_kernel, dim3((w + kTW - 1) / kTW, (h + kTH - 1) / kTH, P), dim3(256), 0, s, M, flow, h, w, m,
                       inv_area, vec);
    CP360_CHECK_HIP();
    return CP360_OK;
}

int launch_upsample(const float* in, int P, int h, int w, float* out, int nh, int nw, float mul, hipStream_t s) {
    hipLaunchKernelGGL(flow_upsample_kernel, dim3((nw + 255) / 256, nh, P), dim3(256), 0, s, (const float2*)in, h, w, (float2*)out,
                       nh, nw, mul);
    CP360_CHECK_HIP();
    return CP360_OK;
}

int check_params(double pyr_scale, int levels, int winsize, int iterations, int poly_n, double poly_sigma, int flags) {
    if (flags != 0) return CP360_ERR_UNSUPPORTED;                  // Gaussian window, initial flow
    if (!(pyr_scale > 0.0 && pyr_scale < 1.0) || levels < 0 || iterations < 1 || !(poly_sigma > 0.0)) return CP360_ERR_BAD_SHAPE;
    if (winsize < 1 || !(winsize & 1) || poly_n < 1) return CP360_ERR_BAD_SHAPE;
    if (winsize / 2 > kMaxBoxM || poly_n > kMaxPolyN) return CP360_ERR_UNSUPPORTED;
    return CP360_OK;
}

struct Geometry {
    int L;
    int h[kMaxLevels + 1], w[kMaxLevels + 1], ksz[kMaxLevels + 1];
    double sigma[kMaxLevels + 1];
};

int geometry(int H, int W, double pyr_scale, int levels, Geometry* g) {
    const int L = cp360_optflow_levels_host(H, W, pyr_scale, levels, kMaxLevels + 1, g->h, g->w, g->ksz, g->sigma);
    if (L < 0) return L;
    g->L = L;
    for (int k = 0; k <= L; ++k)
        if (g->ksz[k] > kMaxKsz) return CP360_ERR_UNSUPPORTED;
    return CP360_OK;
}

// workspace (floats): level images [F + 1, n] | R [F + 1, 5, n] | M [F, 5, n] (first the horizontal blur [F + 1, n]) | the flow
// of the odd levels [F, n1, 2]; the flow of the even levels lives in the output
struct WorkLayout {
    size_t img, R, M, fl, total;
};

WorkLayout work_layout(int F, int H, int W, const Geometry& g) {
    const size_t n = (size_t)H * W, n1 = g.L >= 1 ? (size_t)g.h[1] * g.w[1] : 0;
    WorkLayout l;
    l.img = 0;
    l.R = l.img + (size_t)(F + 1) * n;
    l.M = l.R + (size_t)(F + 1) * 5 * n;
    l.fl = l.M + (size_t)F * 5 * n;
    l.total = l.fl + (size_t)F * n1 * 2;
    return l;
}

}  // namespace

// ------------------------------------------------------------------ C ABI: host tables
extern "C" int cp360_optflow_levels_host(int H, int W, double pyr_scale, int levels, int cap, int* hs, int* ws, int* ksz,
                                         double* sigma) {
    if (H <= 0 || W <= 0 || levels < 0 || !(pyr_scale > 0.0 && pyr_scale < 1.0) || cap < 0) return CP360_ERR_BAD_SHAPE;
    int k = 0;
    double scale = 1.0;
    while (k < levels) {
        scale *= pyr_scale;
        if (W * scale < 32 || H * scale < 32) break;
        ++k;
    }
    const int L = k;
    if (!hs && !ws && !ksz && !sigma) return L;
    if (L + 1 > cap) return CP360_ERR_UNSUPPORTED;
    for (k = 0; k <= L; ++k) {
        scale = 1.0;
        for (int i = 0; i < k; ++i) scale *= pyr_scale;
        const double sg = (1.0 / scale - 1.0) * 0.5;
        int sz = cv_round(sg * 5) | 1;
        if (sz < 3) sz = 3;
        if (hs) hs[k] = cv_round(H * scale);
        if (ws) ws[k] = cv_round(W * scale);
        if (ksz) ksz[k] = sz;
        if (sigma) sigma[k] = sg;
    }
    return L;
}

extern "C" int cp360_optflow_gauss_host(int ksz, double sigma, float* taps) {
    if (!taps) return CP360_ERR_NULL;
    if (ksz < 1 || !(ksz & 1)) return CP360_ERR_BAD_SHAPE;
    if (!(sigma > 0.0)) {                                          // level 0: the fixed small kernel
        if (ksz != 3) return CP360_ERR_BAD_SHAPE;
        taps[0] = 0.25f;
        taps[1] = 0.5f;
        taps[2] = 0.25f;
        return CP360_OK;
    }
    const int r = ksz / 2;
    double sum = 0.0;
    for (int i = 0; i < ksz; ++i) sum += exp(-(double)(i - r) * (i - r) / (2.0 * sigma * sigma));
    for (int i = 0; i < ksz; ++i) taps[i] = (float)(exp(-(double)(i - r) * (i - r) / (2.0 * sigma * sigma)) / sum);
    return CP360_OK;
}

extern "C" int cp360_optflow_poly_tables_host(int n, double sigma, float* g, float* xg, float* xxg, float* ig) {
    if (!g || !xg || !xxg || !ig) return CP360_ERR_NULL;
    if (n < 1 || !(sigma > 0.0)) return CP360_ERR_BAD_SHAPE;
    if (n > kMaxPolyN) return CP360_ERR_UNSUPPORTED;
    double gd[2 * kMaxPolyN + 1], sum = 0.0;
    for (int x = -n; x <= n; ++x) sum += exp(-(double)x * x / (2.0 * sigma * sigma));
    for (int x = -n; x <= n; ++x) gd[x + n] = exp(-(double)x * x / (2.0 * sigma * sigma)) / sum;
    // G = sum g(x) g(y) b b^T, b = (1, x, y, x^2, y^2, xy); A = [G | I] reduced by Gauss-Jordan with partial pivoting
    double A[6][12];
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 12; ++j) A[i][j] = j == i + 6 ? 1.0 : 0.0;
    for (int y = -n; y <= n; ++y)
        for (int x = -n; x <= n; ++x) {
            const double wgt = gd[x + n] * gd[y + n];
            const double b[6] = {1.0, (double)x, (double)y, (double)x * x, (double)y * y, (double)x * y};
            for (int i = 0; i < 6; ++i)
                for (int j = 0; j < 6; ++j) A[i][j] += wgt * b[i] * b[j];
        }
    for (int c = 0; c < 6; ++c) {
        int piv = c;
        for (int r = c + 1; r < 6; ++r)
            if (fabs(A[r][c]) > fabs(A[piv][c])) piv = r;
        if (A[piv][c] == 0.0) return CP360_ERR_BAD_SHAPE;
        for (int j = 0; j < 12; ++j) {
            const double t = A[c][j];
            A[c][j] = A[piv][j];
            A[piv][j] = t;
        }
        const double d = A[c][c];
        for (int j = 0; j < 12; ++j) A[c][j] /= d;
        for (int r = 0; r < 6; ++r) {
            if (r == c) continue;
            const double f = A[r][c];
            for (int j = 0; j < 12; ++j) A[r][j] -= f * A[c][j];
        }
    }
    for (int x = -n; x <= n; ++x) {
        g[x + n] = (float)gd[x + n];
        xg[x + n] = (float)(x * gd[x + n]);
        xxg[x + n] = (float)((double)x * x * gd[x + n]);
    }
    ig[0] = (float)A[1][6 + 1];
    ig[1] = (float)A[0][6 + 3];
    ig[2] = (float)A[3][6 + 3];
    ig[3] = (float)A[5][6 + 5];
    return CP360_OK;
}

// ------------------------------------------------------------------ C ABI: stages
extern "C" int cp360_optflow_gray(const uint8_t* rgb, float* gray, long long n_pixels, void* stream) {
    if (!rgb || !gray) return CP360_ERR_NULL;
    if (n_pixels <= 0) return CP360_ERR_BAD_SHAPE;
    const long long blocks = (n_pixels + 255) / 256;
    hipLaunchKernelGGL(gray_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, (hipStream_t)stream, rgb, gray,
                       n_pixels);
    CP360_CHECK_HIP();
    return CP360_OK;
}

extern "C" int cp360_optflow_pyr_level(const float* gray, int N, int H, int W, int ksz, double sigma, float* out, int lh, int lw,
                                       float* tmp, void* stream) {
    if (!gray || !out || !tmp) return CP360_ERR_NULL;
    if (bad_image(N, H, W) || lh <= 0 || lw <= 0) return CP360_ERR_BAD_SHAPE;
    if (big_image(N, H, W) || big_image(N, lh, lw)) return CP360_ERR_UNSUPPORTED;
    GaussTaps taps;
    const int st = gauss_taps(ksz, sigma, &taps);
    if (st != CP360_OK) return st;
    return launch_pyr_level(gray, N, H, W, taps, ksz, out, lh, lw, tmp, (hipStream_t)stream);
}

extern "C" int cp360_optflow_poly_exp(const float* img, int N, int h, int w, int poly_n, double poly_sigma, float* R,
                                      void* stream) {
    if (!img || !R) return CP360_ERR_NULL;
    if (bad_image(N, h, w)) return CP360_ERR_BAD_SHAPE;
    if (big_image(N, h, w)) return CP360_ERR_UNSUPPORTED;
    PolyTabs tabs;
    const int st = poly_tabs(poly_n, poly_sigma, &tabs);
    if (st != CP360_OK) return st;
    return launch_poly_exp(img, N, h, w, poly_n, tabs, R, (hipStream_t)stream);
}

extern "C" int cp360_optflow_matrices(const float* R0, const float* R1, size_t r_stride, const float* flow, float* M, int P, int h,
                                      int w, void* stream) {
    if (!R0 || !R1 || !flow || !M) return CP360_ERR_NULL;
    if (bad_image(P, h, w)) return CP360_ERR_BAD_SHAPE;
    if (big_image(P, h, w)) return CP360_ERR_UNSUPPORTED;
    if (P > 1 && r_stride < (size_t)5 * h * w) return CP360_ERR_BAD_SHAPE;
    return launch_matrices(R0, R1, r_stride, flow, M, P, h, w, (hipStream_t)stream);
}

extern "C" int cp360_optflow_blur_solve(const float* M, float* flow, int P, int h, int w, int winsize, void* stream) {
    if (!M || !flow) return CP360_ERR_NULL;
    if (bad_image(P, h, w) || winsize < 1 || !(winsize & 1)) return CP360_ERR_BAD_SHAPE;
    if (big_image(P, h, w) || winsize / 2 > kMaxBoxM) return CP360_ERR_UNSUPPORTED;
    return launch_blur_solve(M, flow, P, h, w, winsize, (hipStream_t)stream);
}

extern "C" int cp360_optflow_flow_upsample(const float* flow, int P, int h, int w, float* out, int h_out, int w_out, float mul,
                                           void* stream) {
    if (!flow || !out) return CP360_ERR_NULL;
    if (bad_image(P, h, w) || h_out <= 0 || w_out <= 0) return CP360_ERR_BAD_SHAPE;
    if (big_image(P, h, w) || big_image(P, h_out, w_out)) return CP360_ERR_UNSUPPORTED;
    return launch_upsample(flow, P, h, w, out, h_out, w_out, mul, (hipStream_t)stream);
}

// ------------------------------------------------------------------ C ABI: the whole flow
extern "C" size_t cp360_optflow_work_bytes(int F, int H, int W, double pyr_scale, int levels) {
    if (bad_image(F, H, W) || big_image(F + 1, H, W)) return 0;
    Geometry g;
    if (geometry(H, W, pyr_scale, levels, &g) != CP360_OK) return 0;
    return work_layout(F, H, W, g).total * sizeof(float);
}

extern "C" int cp360_optflow_farneback(const float* gray, int F, int H, int W, double pyr_scale, int levels, int winsize,
                                       int iterations, int poly_n, double poly_sigma, int flags, float* flow, void* work,
                                       size_t work_bytes, void* stream) {
    int st = check_params(pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags);
    if (st != CP360_OK) return st;
    if (!gray || !flow || !work) return CP360_ERR_NULL;
    if (bad_image(F, H, W)) return CP360_ERR_BAD_SHAPE;
    if (big_image(F + 1, H, W)) return CP360_ERR_UNSUPPORTED;
    if (!aligned16(work)) return CP360_ERR_ALIGN;
    Geometry g;
    st = geometry(H, W, pyr_scale, levels, &g);
    if (st != CP360_OK) return st;
    const WorkLayout l = work_layout(F, H, W, g);
    if (work_bytes < l.total * sizeof(float)) return CP360_ERR_BAD_SHAPE;
    PolyTabs tabs;
    st = poly_tabs(poly_n, poly_sigma, &tabs);
    if (st != CP360_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    float* base = (float*)work;
    float *img = base + l.img, *R = base + l.R, *M = base + l.M, *fl_odd = base + l.fl;
    const float up = (float)(1.0 / pyr_scale);
    float* prev = nullptr;
    for (int k = g.L; k >= 0; --k) {
        const int h = g.h[k], w = g.w[k];
        const size_t n = (size_t)h * w;
        GaussTaps taps;
        st = gauss_taps(g.ksz[k], g.sigma[k], &taps);
        if (st != CP360_OK) return st;
        st = launch_pyr_level(gray, F + 1, H, W, taps, g.ksz[k], img, h, w, M, s);      // M is free here: the blur's scratch
        if (st != CP360_OK) return st;
        st = launch_poly_exp(img, F + 1, h, w, poly_n, tabs, R, s);
        if (st != CP360_OK) return st;
        float* cur = (k & 1) ? fl_odd : flow;
        if (!prev) {
            if (hipMemsetAsync(cur, 0, (size_t)F * n * 2 * sizeof(float), s) != hipSuccess) return CP360_ERR_HIP;
        } else {
            st = launch_upsample(prev, F, g.h[k + 1], g.w[k + 1], cur, h, w, up, s);
            if (st != CP360_OK) return st;
        }
        for (int it = 0; it < iterations; ++it) {
            st = launch_matrices(R, R + 5 * n, 5 * n, cur, M, F, h, w, s);
            if (st != CP360_OK) return st;
            st = launch_blur_solve(M, cur, F, h, w, winsize, s);
            if (st != CP360_OK) return st;
        }
        prev = cur;
    }
    return CP360_OK;
}
