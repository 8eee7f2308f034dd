// The sphere geometry of an equirectangular image, shared by stabilize.hip (K11), viewport.hip (K12), sphere_eval.hip (K14),
// fixations.hip (K15), headtrack.hip (K17), egomotion.hip (K23), streaming.hip (K24) and, through sphere_eval.hip's resampler, suploss.hip (K18): the one definition of dir, pix, the rotation of a direction, the (cos, sin) tables
// of the pixel centres and the bilinear sample that wraps in x and clamps in y (DESIGN.md "K11" geometry;
// tests/stabilize_restate.py restates it); and what their kernels and entry points repeat: the von Mises-Fisher term, whether a
// direction lies in a camera's view, the lens of a view as a value or a table, the items of a frame in CSR form, the ordered sum of a 256-thread workgroup, how a caller's
// workspace is opened and the dispatch on the pixel type (DESIGN.md "What the sphere kernels share").
//
//     theta = (2 (x + 1/2) / W - 1) pi        phi = (1 - 2 (y + 1/2) / H) pi / 2        dir = (cos phi cos theta, sin phi, cos phi sin theta)
//     pix(q): theta = atan2(q_z, q_x), phi = asin(clamp(q_y, -1, 1)), x = (theta / pi + 1) W / 2 - 1/2, y = (1 - phi / (pi / 2)) H / 2 - 1/2
//
// Every term is f32 with plain operators: the including file switches contraction off before it includes this header
// (#pragma clang fp contract(off)), so that a float32 restatement follows the kernels operation by operation.  Everything here
// has internal linkage: each file that includes it compiles its own copy.
#pragma once
#include "common.h"
#include "../../include/cp360.h"

#include <math.h>
#include <type_traits>

#pragma clang fp contract(off)

namespace {

constexpr float kInvPi = 0.318309886183790671538f;
constexpr float kTwoOverPi = 0.636619772367581343076f;

struct Rot {
    float r00, r01, r02, r10, r11, r12, r20, r21, r22;
};

// direction of pixel centre (x, y) from its column's (cos, sin) theta and its row's (cos, sin) phi
__device__ __forceinline__ void stab_dir(const float2 cs_theta, const float2 cs_phi, float& px, float& py, float& pz) {
    px = cs_phi.x * cs_theta.x;
    py = cs_phi.y;
    pz = cs_phi.x * cs_theta.y;
}

__device__ __forceinline__ void stab_rotate(const Rot& R, float px, float py, float pz, float& qx, float& qy, float& qz) {
    qx = R.r00 * px + R.r01 * py + R.r02 * pz;
    qy = R.r10 * px + R.r11 * py + R.r12 * pz;
    qz = R.r20 * px + R.r21 * py + R.r22 * pz;
}

// pix(q) in pixel-index units; half_w = W / 2, half_h = H / 2
__device__ __forceinline__ void stab_pix(float qx, float qy, float qz, float half_w, float half_h, float& sx, float& sy) {
    const float theta = atan2f(qz, qx);
    const float phi = asinf(fminf(fmaxf(qy, -1.f), 1.f));
    sx = (theta * kInvPi + 1.f) * half_w - 0.5f;
    sy = (1.f - phi * kTwoOverPi) * half_h - 0.5f;
}

__device__ __forceinline__ Rot load_rot(const float* R) {
    Rot r;
    r.r00 = R[0]; r.r01 = R[1]; r.r02 = R[2];
    r.r10 = R[3]; r.r11 = R[4]; r.r12 = R[5];
    r.r20 = R[6]; r.r21 = R[7]; r.r22 = R[8];
    return r;
}

__device__ __forceinline__ float to_f32(float v) { return v; }
__device__ __forceinline__ float to_f32(uint8_t v) { return (float)v; }
__device__ __forceinline__ void store_px(float* p, float v) { *p = v; }
__device__ __forceinline__ void store_px(uint8_t* p, float v) { *p = (uint8_t)fminf(fmaxf(rintf(v), 0.f), 255.f); }

// The C channels of the H x W image `img` at the real position (sx, sy), bilinear: four taps, columns wrap modulo W, rows
// clamp to 0 .. H - 1, top + ty (bot - top).  A non-finite position (a non-finite R) samples inside the frame.
// sphere_sample_f32 leaves the C values in f32, not rounded for u8 images (K21 adds them up); sphere_sample stores them.
template <typename T, int C>
__device__ __forceinline__ void sphere_sample_f32(const T* img, int H, int W, float sx, float sy, float* v) {
    if (!(fabsf(sx) <= (float)W)) sx = 0.f;                            // a non-finite R: stay inside the frame
    sy = fminf(fmaxf(sy, 0.f), (float)(H - 1));                        // fmaxf(NaN, 0) = 0
    const float x0f = floorf(sx), y0f = floorf(sy);
    const float tx = sx - x0f, ty = sy - y0f;
    int x0 = (int)x0f % W;
    if (x0 < 0) x0 += W;
    const int x1 = x0 + 1 == W ? 0 : x0 + 1;
    const int y0 = (int)y0f;
    const int y1 = y0 + 1 < H ? y0 + 1 : H - 1;
    const T* p00 = img + ((size_t)y0 * W + x0) * C;
    const T* p01 = img + ((size_t)y0 * W + x1) * C;
    const T* p10 = img + ((size_t)y1 * W + x0) * C;
    const T* p11 = img + ((size_t)y1 * W + x1) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float v00 = to_f32(p00[c]), v01 = to_f32(p01[c]), v10 = to_f32(p10[c]), v11 = to_f32(p11[c]);
        const float top = v00 + tx * (v01 - v00);
        const float bot = v10 + tx * (v11 - v10);
        v[c] = top + ty * (bot - top);
    }
}

template <typename T, int C>
__device__ __forceinline__ void sphere_sample(const T* img, int H, int W, float sx, float sy, T* o) {
    float v[C];
    sphere_sample_f32<T, C>(img, H, W, sx, sy, v);
#pragma unroll
    for (int c = 0; c < C; ++c) store_px(o + c, v[c]);
}

// ------------------------------------------------------------------ tables
// tabx f32 [W][2] = (cos, sin) theta, taby f32 [H][2] = (cos, sin) phi: cospi / sinpi of the exact fraction in double
__global__ __launch_bounds__(256) void stab_tables_kernel(float2* __restrict__ tabx, float2* __restrict__ taby, int H, int W) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < W) {
        const double t = (double)(2 * i + 1) / (double)W - 1.0;              // theta / pi
        tabx[i] = make_float2((float)cospi(t), (float)sinpi(t));
    } else if (i < W + H) {
        const int y = i - W;
        const double t = 0.5 * (1.0 - (double)(2 * y + 1) / (double)H);      // phi / pi
        taby[y] = make_float2((float)cospi(t), (float)sinpi(t));
    }
}

// ------------------------------------------------------------------ the von Mises-Fisher term of K12c, K12d and K15b
__device__ __forceinline__ float vmf(float kappa, float px, float py, float pz, float qx, float qy, float qz) {
    const float dot = px * qx + py * qy + pz * qz;
    return expf(kappa * (dot - 1.f));
}

// ------------------------------------------------------------------ the view of a camera on the panorama (K17; K12b's decision)
// whether every entry of R is finite: one sum, which a single non-finite entry leaves non-finite
__device__ __forceinline__ bool rot_finite(const Rot& R) {
    const float s = fabsf(R.r00) + fabsf(R.r01) + fabsf(R.r02) + fabsf(R.r10) + fabsf(R.r11) + fabsf(R.r12) + fabsf(R.r20) +
                    fabsf(R.r21) + fabsf(R.r22);
    return isfinite(s);
}

// A camera is K12's: camera-to-world, columns (forward, up, right).  view_rot loads one for view_inside: a camera with a
// non-finite entry comes back all NaN, so that every comparison below fails - its view is empty.
__device__ __forceinline__ Rot view_rot(const float* R) {
    Rot r = load_rot(R);
    if (!rot_finite(r)) r.r00 = r.r01 = r.r02 = r.r10 = r.r11 = r.r12 = r.r20 = r.r21 = r.r22 = NAN;
    return r;
}

__device__ __forceinline__ bool view_rot_finite(const Rot& r) { return r.r00 == r.r00; }   // of view_rot's result

// the view-frame terms of the direction p under the camera R: d = R^T p = (d_f, d_u, d_r) -> d_f, au = |d_r / d_f|, av =
// |d_u / d_f|.  K12b's decision and K17's are comparisons of these three, so both see the same bits.
__device__ __forceinline__ void view_terms(const Rot& R, float px, float py, float pz, float& df, float& au, float& av) {
    df = R.r00 * px + R.r10 * py + R.r20 * pz;
    const float du = R.r01 * px + R.r11 * py + R.r21 * pz;
    const float dr = R.r02 * px + R.r12 * py + R.r22 * pz;
    au = fabsf(dr / df);
    av = fabsf(du / df);
}

// whether the direction p lies in the view of the camera R (from view_rot) with the tangents tx = tan(hfov / 2), ty = tx h / w:
// inside <=> d_f > 0, |u| <= tx, |v| <= ty
__device__ __forceinline__ bool view_inside(const Rot& R, float tx, float ty, float px, float py, float pz) {
    float df, au, av;
    view_terms(R, px, py, pz, df, au, av);
    return df > 0.f && au <= tx && av <= ty;
}

// ------------------------------------------------------------------ the lens of a view, as a value a kernel asks for (K22)
// A lens is (tx, ty, b, 0): the two tangents and K12b's border in tangent units.  A kernel template takes either source and
// calls at(frame).  LensFixed is one lens for every frame, by value in the kernel's arguments; LensTable is a lens per frame,
// f32 [N][4] on the device, 16-byte aligned: one 16-byte load at an address that a workgroup (a wave) shares.
struct LensFixed {
    float tx, ty, b;
    __device__ __forceinline__ float4 at(int) const { return make_float4(tx, ty, b, 0.f); }
};

struct LensTable {
    const float4* lens;
    __device__ __forceinline__ float4 at(int frame) const { return lens[frame]; }
};

// ------------------------------------------------------------------ items in CSR form (K15's points, K17's cameras)
__device__ __forceinline__ int fix_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the items of frame f, inside 0 .. N whatever the offsets hold
__device__ __forceinline__ void fix_range(const int* __restrict__ offsets, int f, int N, int& k0, int& k1) {
    k0 = fix_clamp(offsets[f], 0, N);
    k1 = fix_clamp(offsets[f + 1], k0, N);
}

// the frame of item k (K17b's pairs, K19b's points): offsets[f] <= k < offsets[f + 1] (empty frames repeat an offset); inside
// 0 .. F - 1 whatever the offsets hold
__device__ __forceinline__ int fix_frame(const int* __restrict__ offsets, int F, int k) {
    int lo = 0, hi = F - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid + 1] > k) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// ------------------------------------------------------------------ the ordered sum of a 256-thread workgroup
// One fixed tree, whose bits the callers see: a wave's 64 values by __shfl_down with offsets 32, 16, .. 1 (lane 0 ends with the
// sum), then lane 0 of each of the four waves leaves it in LDS and the slots add up as ((r0 + r1) + r2) + r3.
template <typename T>
__device__ __forceinline__ T wave_sum_down(T v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// slot[k * stride] = wave k's sum
template <typename T>
__device__ __forceinline__ T waves4_sum(const T* slot, int stride) {
    return ((slot[0] + slot[stride]) + slot[2 * stride]) + slot[3 * stride];
}

// ------------------------------------------------------------------ host side
// The tables at the head of a workspace: tab_bytes = cp360_stab_work_bytes(0, H, W).  open_tabs is how an entry point takes the
// caller's workspace: a misaligned one is CP360_ERR_ALIGN, one below `need` bytes CP360_ERR_BAD_SHAPE, then the tables are
// launched and t points at them.  An entry point with a check between the two halves calls them itself.
struct SphereTabs {
    const float2 *x, *y;
};

size_t tab_bytes(int H, int W) { return align16((size_t)W * sizeof(float2)) + align16((size_t)H * sizeof(float2)); }

int check_work(const void* work, size_t work_bytes, size_t need) {
    if (!aligned16(work)) return CP360_ERR_ALIGN;
    return work_bytes < need ? CP360_ERR_BAD_SHAPE : CP360_OK;
}

int launch_tables(void* work, int H, int W, hipStream_t s, SphereTabs* t) {
    float2* x = (float2*)work;
    float2* y = (float2*)((char*)work + align16((size_t)W * sizeof(float2)));
    hipLaunchKernelGGL(stab_tables_kernel, dim3((H + W + 255) / 256), dim3(256), 0, s, x, y, H, W);
    CP360_CHECK_HIP();
    t->x = x;
    t->y = y;
    return CP360_OK;
}

int open_tabs(void* work, size_t work_bytes, size_t need, int H, int W, hipStream_t s, SphereTabs* t) {
    const int st = check_work(work, work_bytes, need);
    return st != CP360_OK ? st : launch_tables(work, H, W, s, t);
}

// the two tangents of a view (K17, K24), tx = tan(hfov / 2), ty = tx aspect in double, each rounded once; false for a view that
// is refused
bool head_tangents(double hfov_rad, double aspect, float* tx, float* ty) {
    if (!(hfov_rad > 0.0) || !(hfov_rad < 3.14159265358979323846) || !(aspect > 0.0)) return false;
    const double t = tan(0.5 * hfov_rad);
    *tx = (float)t;
    *ty = (float)(t * aspect);
    return isfinite(*tx) && isfinite(*ty);
}

// f(T(), integral_constant<int, C>()) for the pixel types of K11c and K12a: u8 x 3 or f32 x 1 .. 4 (the caller has checked)
template <typename F>
int dispatch_pixels(int dtype, int C, F f) {
    if (dtype == CP360_U8) return f(uint8_t(), std::integral_constant<int, 3>());
    switch (C) {
        case 1: return f(float(), std::integral_constant<int, 1>());
        case 2: return f(float(), std::integral_constant<int, 2>());
        case 3: return f(float(), std::integral_constant<int, 3>());
        default: return f(float(), std::integral_constant<int, 4>());
    }
}

}  // namespace
