// K17: ground truth from head tracking.  A headset logs where the head points, not where the eyes rest: what a viewer saw is the
// window of the headset, the view of a camera (K12's convention: R f32 [3, 3] camera-to-world, columns forward / up / right).  A
// video's viewers are N cameras in CSR form, as K15's points: offsets int32 [F + 1], the cameras of frame f are offsets[f] ..
// offsets[f + 1] - 1.  The specification is the package's own, DESIGN.md "K17"; tests/headtrack_restate.py restates it.
//
//   inside      sphere.h's view_inside, K12b's decision: p = dir(x, y) is in the view of R with the tangents (tx, ty) <=> d_f > 0,
//               |d_r / d_f| <= tx, |d_u / d_f| <= ty with (d_f, d_u, d_r) = R^T p, f32 in K12b's order; tx = tan(hfov / 2), ty = tx
//               aspect in double on the host, rounded to f32 once.  A camera with a non-finite entry has an empty view.
//   footprints  counts[f, y, x] = the number of frame f's cameras whose view holds dir(x, y); n_views[f] = the number of its finite
//               cameras.  counts / n_views is the share of the viewers who had the pixel in view: the ground-truth map.
//   agreement   of a camera Rc[f] per frame (with a view of its own) and every viewer k of that frame, weighted by the rows'
//               integer weights a_y (K13's solid-angle table, or 1024 everywhere): inter[k] = sum a_y [in_cam and in_view(k)],
//               uni[k] = sum a_y [in_cam or in_view(k)]; inter / uni is the intersection over union of the two windows on the sphere
//
// Launches, on the caller's stream, no host synchronisation, no atomics; exact integers, so a frame's counts and a pair's sums do
// not depend on F, N or their place in the batch:
//   K17a  footprints: grid (ceil(P / 256), F), a pixel per thread; the frame's cameras staged in LDS kHeadChunk at a time, every
//         lane reads the same address (a broadcast), the loop is wave-uniform
//   K17b  agreement: a wave per pair, four pairs per workgroup; the wave finds its frame by a search in offsets, strides over the
//         pixels with int32 partial sums (at most 2^15 pixels of weight 1024 a lane) and adds them up in 64 bits by
//         wave_sum_down; no LDS, no barrier
//   K22c  K17b's kernel with the camera's tangents per frame, from K22's lens table (DESIGN.md "K22"): one kernel template over
//         sphere.h's lens sources serves both
#pragma clang fp contract(off)
#include "roc.h"

#include <math.h>

namespace {

constexpr int kHeadChunk = 64;               // K17a: cameras staged at a time, by the workgroup's first wave
static_assert(kHeadChunk <= 64, "K17a counts the finite cameras in the one wave that stages them");
constexpr int kHeadPairs = 4;                // K17b: pairs (waves) per workgroup
constexpr int kMaxWeight = 1024;

// ------------------------------------------------------------------ K17a: footprints
// grid (ceil(P / 256), F), 256 threads
__global__ __launch_bounds__(256) void head_footprints_kernel(const float* __restrict__ R, const int* __restrict__ offsets, int N,
                                                              const float2* __restrict__ tabx, const float2* __restrict__ taby,
                                                              int* __restrict__ counts, int* __restrict__ n_views, int h, int w,
                                                              float tx, float ty) {
    __shared__ Rot tile[kHeadChunk];
    const int P = h * w, tid = threadIdx.x, f = blockIdx.y;
    const int i = blockIdx.x * 256 + tid;
    int k0, k1;
    fix_range(offsets, f, N, k0, k1);
    float px = 1.f, py = 0.f, pz = 0.f;                                // a thread past the frame keeps the barriers' company and stores nothing
    if (i < P) {
        const int y = i / w, x = i - y * w;
        stab_dir(tabx[x], taby[y], px, py, pz);
    }
    int acc = 0, finite = 0;
    for (long long t0 = k0; t0 < k1; t0 += kHeadChunk) {               // k0, k1 are the workgroup's: the barriers are uniform
        const long long k = t0 + tid;
        if (tid < kHeadChunk && k < k1) {
            const Rot r = view_rot(R + k * 9);
            finite += view_rot_finite(r);
            tile[tid] = r;
        }
        __syncthreads();
        const int n = k1 - t0 < kHeadChunk ? (int)(k1 - t0) : kHeadChunk;
        for (int c = 0; c < n; ++c) acc += view_inside(tile[c], tx, ty, px, py, pz);
        __syncthreads();
    }
    if (i < P) counts[(size_t)f * P + i] = acc;                        // a frame without cameras: zeros
    if (blockIdx.x == 0 && tid < 64) {                                 // the first wave staged every camera
        finite = wave_sum_down(finite);
        if (tid == 0) n_views[f] = finite;
    }
}

// ------------------------------------------------------------------ K17b, K22c: agreement
// grid ceil(N / 4), 256 threads; the frame of pair k is sphere.h's fix_frame.  The camera's tangents (ctx, cty) are the first two
// values of its lens at that frame - sphere.h's LensFixed for the one view of K17b, LensTable for K22's table (one 16-byte load,
// uniform over the wave); the viewers' window (tx, ty) is the call's.  A tangent that is not finite fails every comparison of
// view_inside: that camera's view is empty.
template <typename Lens>
__global__ __launch_bounds__(64 * kHeadPairs) void head_agreement_kernel(const float* __restrict__ Rc, const Lens cam_lens,
                                                                         const float* __restrict__ R, const int* __restrict__ offsets,
                                                                         int N, int F, const float2* __restrict__ tabx,
                                                                         const float2* __restrict__ taby, const int* __restrict__ weights,
                                                                         long long* __restrict__ inter, long long* __restrict__ uni, int h,
                                                                         int w, float tx, float ty) {
    const int lane = threadIdx.x & 63;
    const long long k = (long long)blockIdx.x * kHeadPairs + (threadIdx.x >> 6);
    if (k >= N) return;                                                // the whole wave; the kernel has no barrier
    const int f = fix_frame(offsets, F, (int)k);
    const float4 L = cam_lens.at(f);
    const float ctx = L.x, cty = L.y;
    const Rot cam = view_rot(Rc + (size_t)f * 9);
    const Rot view = view_rot(R + k * 9);
    const int P = h * w;
    int x = lane % w, y = lane / w;
    int si = 0, su = 0;
    for (int i = lane; i < P; i += 64) {
        float px, py, pz;
        stab_dir(tabx[x], taby[y], px, py, pz);
        const bool c = view_inside(cam, ctx, cty, px, py, pz), v = view_inside(view, tx, ty, px, py, pz);
        const int a = fix_clamp(weights[y], 0, kMaxWeight);
        si += c && v ? a : 0;
        su += c || v ? a : 0;
        x += 64;
        while (x >= w) {
            x -= w;
            ++y;
        }
    }
    const long long ti = wave_sum_down((long long)si), tu = wave_sum_down((long long)su);
    if (lane == 0) {
        inter[k] = ti;
        uni[k] = tu;
    }
}

// ------------------------------------------------------------------ host side
// the viewers: R may be NULL when there are none
int head_cameras(const float* R, const int32_t* offsets, long long N, int F, int h, int w) {
    if (!offsets || (!R && N > 0)) return CP360_ERR_NULL;
    const int st = roc_args(F, h, w);
    if (st != CP360_OK) return st;
    if (N < 0) return CP360_ERR_BAD_SHAPE;
    if (N >= (1LL << 31)) return CP360_ERR_UNSUPPORTED;
    if ((((uintptr_t)R | (uintptr_t)offsets) & 3) != 0) return CP360_ERR_ALIGN;
    return CP360_OK;
}

// K17b and K22c: the checks of both entry points in the order of their statuses, the tables and the launch.  cam_st is what the
// entry point found about the camera's lens: CP360_OK, or the status to return where these checks reach it.
template <typename Lens>
int head_agreement(const float* Rc, Lens cam_lens, int cam_st, const float* R, const int32_t* offsets, long long N, int F, int h, int w,
                   double hfov_rad, double aspect, const int32_t* weights, long long* inter, long long* uni, void* work,
                   size_t work_bytes, void* stream) {
    if (!Rc || !weights || !work || ((!inter || !uni) && N > 0) || cam_st == CP360_ERR_NULL) return CP360_ERR_NULL;
    int st = head_cameras(R, offsets, N, F, h, w);
    if (st != CP360_OK) return st;
    float tx, ty;
    if (cam_st == CP360_ERR_BAD_SHAPE || !head_tangents(hfov_rad, aspect, &tx, &ty)) return CP360_ERR_BAD_SHAPE;
    if ((((uintptr_t)Rc | (uintptr_t)weights) & 3) != 0 || cam_st == CP360_ERR_ALIGN || (((uintptr_t)inter | (uintptr_t)uni) & 7) != 0)
        return CP360_ERR_ALIGN;
    st = check_work(work, work_bytes, tab_bytes(h, w));
    if (st != CP360_OK || N == 0) return st;                           // no pairs: nothing to launch
    hipStream_t s = (hipStream_t)stream;
    SphereTabs t;
    st = launch_tables(work, h, w, s, &t);
    if (st != CP360_OK) return st;
    hipLaunchKernelGGL(head_agreement_kernel<Lens>, dim3((unsigned)((N + kHeadPairs - 1) / kHeadPairs)), dim3(64 * kHeadPairs), 0, s, Rc,
                       cam_lens, R, (const int*)offsets, (int)N, F, t.x, t.y, (const int*)weights, inter, uni, h, w, tx, ty);
    CP360_CHECK_HIP();
    return CP360_OK;
}

}  // namespace

// ------------------------------------------------------------------ C ABI
extern "C" int cp360_head_footprints(const float* R, const int32_t* offsets, long long N, int F, int h, int w, double hfov_rad,
                                     double aspect, int32_t* counts, int32_t* n_views, void* work, size_t work_bytes, void* stream) {
    if (!counts || !n_views || !work) return CP360_ERR_NULL;
    int st = head_cameras(R, offsets, N, F, h, w);
    if (st != CP360_OK) return st;
    float tx, ty;
    if (!head_tangents(hfov_rad, aspect, &tx, &ty)) return CP360_ERR_BAD_SHAPE;
    if ((((uintptr_t)counts | (uintptr_t)n_views) & 3) != 0) return CP360_ERR_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    SphereTabs t;
    st = open_tabs(work, work_bytes, tab_bytes(h, w), h, w, s, &t);
    if (st != CP360_OK) return st;
    hipLaunchKernelGGL(head_footprints_kernel, dim3((h * w + 255) / 256, F), dim3(256), 0, s, R, (const int*)offsets, (int)N, t.x,
                       t.y, (int*)counts, (int*)n_views, h, w, tx, ty);
    CP360_CHECK_HIP();
    return CP360_OK;
}

extern "C" int cp360_head_agreement(const float* Rc, double cam_hfov_rad, double cam_aspect, const float* R, const int32_t* offsets,
                                    long long N, int F, int h, int w, double hfov_rad, double aspect, const int32_t* weights,
                                    long long* inter, long long* uni, void* work, size_t work_bytes, void* stream) {
    LensFixed cam = {};
    const int cam_st = head_tangents(cam_hfov_rad, cam_aspect, &cam.tx, &cam.ty) ? CP360_OK : CP360_ERR_BAD_SHAPE;
    return head_agreement(Rc, cam, cam_st, R, offsets, N, F, h, w, hfov_rad, aspect, weights, inter, uni, work, work_bytes, stream);
}

// K22c: the cameras' lenses in place of their view
extern "C" int cp360_head_agreement_zoom(const float* Rc, const float* cam_lens, const float* R, const int32_t* offsets, long long N,
                                         int F, int h, int w, double hfov_rad, double aspect, const int32_t* weights, long long* inter,
                                         long long* uni, void* work, size_t work_bytes, void* stream) {
    const int cam_st = !cam_lens ? CP360_ERR_NULL : (!aligned16(cam_lens) ? CP360_ERR_ALIGN : CP360_OK);
    return head_agreement(Rc, LensTable{(const float4*)cam_lens}, cam_st, R, offsets, N, F, h, w, hfov_rad, aspect, weights, inter, uni,
                          work, work_bytes, stream);
}
