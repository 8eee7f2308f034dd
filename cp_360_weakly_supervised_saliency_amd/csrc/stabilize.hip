// K11: 360-degree stabilisation of equirectangular video - the camera rotation of every frame pair fitted to the optical flow
// K10 computes (K11a), the flow a rotation induces (K11b) and the frames re-rendered under a rotation (K11c).  The reference has
// no counterpart (its README leaves moving cameras to the user); the specification is the package's own, DESIGN.md "K11", and
// tests/stabilize_restate.py restates it in float64.
//
// Geometry (the conventions of utils/sph_utils.py: xy2angle, to_3dsphere).  Pixel (x, y) of an H x W image has its centre at
// (x + 1/2, y + 1/2):
//     theta = (2 (x + 1/2) / W - 1) pi        phi = (1 - 2 (y + 1/2) / H) pi / 2        dir = (cos phi cos theta, sin phi, cos phi sin theta)
//     pix(q): theta = atan2(q_z, q_x), phi = asin(clamp(q_y, -1, 1)), x = (theta / pi + 1) W / 2 - 1/2, y = (1 - phi / (pi / 2)) H / 2 - 1/2
// dir of a pixel centre comes from two tables, (cos, sin) theta per column and (cos, sin) phi per row: evaluated in double as
// cospi / sinpi of the exact fractions and rounded to f32 once, by a kernel at the head of every call (the tables live in the
// caller's workspace).  dir of a displaced position (x + dx, y + dy) is the angle sum of the table entry with sincosf of the
// displacement's angle, which continues smoothly over a pole.  Every per-pixel term is f32 with plain operators and contraction
// off (as metrics.hip), so the restatement follows it operation by operation; every sum is f64 in a fixed order.
//
// K11a, per pair: R_0 = I; iteration k: q = R_k p, d = p_f - q, r2 = |d|^2, w = cos phi (k = 0) or cos phi / (1 + r2 / c_k^2)^2,
// N = sum w (I - q q^T), b = sum w (q x p_f); delta = N^-1 b, R_k+1 = exp([delta]x) R_k; c_1 = max(c_min, 2 s), c_k+1 = max(c_min,
// c_k / 2), s = sqrt(sum w r2 / sum w).  Two launches per iteration for all pairs: 256 threads x 8 pixels give one f64 partial
// of 11 sums per workgroup (registers, wave shuffles, LDS across the 4 waves); one wave per pair adds the partials (lane l takes
// l, l + 64, ... in order, then the shuffle tree), solves and updates the pair's state in the workspace.  No atomics, no host
// synchronisation, results independent of the batch size.
#pragma clang fp contract(off)

#include "sphere.h"

namespace {

constexpr int kFitPx = 8;                    // pixels per thread of the accumulation
constexpr int kFitBlock = 256 * kFitPx;      // pixels per workgroup = per partial
constexpr int kSums = 11;                    // Nxx Nxy Nxz Nyy Nyz Nzz bx by bz sum_w sum_w_r2
constexpr int kPartial = 12;                 // doubles per partial (padded)
constexpr int kState = 16;                   // doubles per pair: R[9], c, dead, 1 / c^2

// ------------------------------------------------------------------ geometry: dir, pix, the rotation and the sampler are sphere.h's
// direction of (x + dx, y + dy): the angle sums theta + dx 2 pi / W and phi - dy pi / H
__device__ __forceinline__ void stab_dir_moved(const float2 cs_theta, const float2 cs_phi, float dx, float dy, float kx, float ky,
                                               float& px, float& py, float& pz) {
    float sa, ca, sb, cb;
    sincosf(dx * kx, &sa, &ca);
    sincosf(-(dy * ky), &sb, &cb);
    const float ct = cs_theta.x * ca - cs_theta.y * sa;
    const float st = cs_theta.y * ca + cs_theta.x * sa;
    const float cp = cs_phi.x * cb - cs_phi.y * sb;
    const float sp = cs_phi.y * cb + cs_phi.x * sb;
    px = cp * ct;
    py = sp;
    pz = cp * st;
}

// ------------------------------------------------------------------ K11a: fit
__global__ __launch_bounds__(64) void stab_fit_init_kernel(double* __restrict__ state, int F, double c_min) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= F) return;
    double* S = state + (size_t)p * kState;
    S[0] = 1.0; S[1] = 0.0; S[2] = 0.0;
    S[3] = 0.0; S[4] = 1.0; S[5] = 0.0;
    S[6] = 0.0; S[7] = 0.0; S[8] = 1.0;
    S[9] = c_min;
    S[10] = 0.0;
    S[11] = 1.0 / (c_min * c_min);
}

// grid (ceil(H W / 2048), F): one partial of 11 f64 sums per workgroup
__global__ __launch_bounds__(256) void stab_fit_accum_kernel(const float2* __restrict__ flow, const float2* __restrict__ tabx,
                                                             const float2* __restrict__ taby, const double* __restrict__ state,
                                                             double* __restrict__ partials, int H, int W, float kx, float ky,
                                                             int first) {
    __shared__ double red[4][kSums];
    const int pair = blockIdx.y, tid = threadIdx.x;
    const int n = H * W;
    const double* S = state + (size_t)pair * kState;
    Rot R;
    R.r00 = (float)S[0]; R.r01 = (float)S[1]; R.r02 = (float)S[2];
    R.r10 = (float)S[3]; R.r11 = (float)S[4]; R.r12 = (float)S[5];
    R.r20 = (float)S[6]; R.r21 = (float)S[7]; R.r22 = (float)S[8];
    const float inv_c2 = (float)S[11];
    const float2* fl = flow + (size_t)pair * n;
    double acc[kSums];
#pragma unroll
    for (int k = 0; k < kSums; ++k) acc[k] = 0.0;
#pragma unroll
    for (int j = 0; j < kFitPx; ++j) {
        const int i = blockIdx.x * kFitBlock + j * 256 + tid;
        if (i >= n) continue;
        const float2 f = fl[i];
        if (!(isfinite(f.x) && isfinite(f.y))) continue;                   // weight 0
        const int y = i / W, x = i - y * W;
        const float2 cst = tabx[x], csp = taby[y];
        float px, py, pz, fx, fy, fz, qx, qy, qz;
        stab_dir(cst, csp, px, py, pz);
        stab_dir_moved(cst, csp, f.x, f.y, kx, ky, fx, fy, fz);
        stab_rotate(R, px, py, pz, qx, qy, qz);
        const float dx = fx - qx, dy = fy - qy, dz = fz - qz;
        const float r2 = dx * dx + dy * dy + dz * dz;
        float w = csp.x;
        if (!first) {
            const float u = 1.f + r2 * inv_c2;
            w = csp.x / (u * u);
        }
        acc[0] += (double)(w * (1.f - qx * qx));
        acc[1] -= (double)(w * (qx * qy));
        acc[2] -= (double)(w * (qx * qz));
        acc[3] += (double)(w * (1.f - qy * qy));
        acc[4] -= (double)(w * (qy * qz));
        acc[5] += (double)(w * (1.f - qz * qz));
        acc[6] += (double)(w * (qy * fz - qz * fy));
        acc[7] += (double)(w * (qz * fx - qx * fz));
        acc[8] += (double)(w * (qx * fy - qy * fx));
        acc[9] += (double)w;
        acc[10] += (double)(w * r2);
    }
#pragma unroll
    for (int k = 0; k < kSums; ++k) acc[k] = wave_sum_down(acc[k]);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < kSums; ++k) red[tid >> 6][k] = acc[k];
    }
    __syncthreads();
    if (tid < kSums) partials[((size_t)pair * gridDim.x + blockIdx.x) * kPartial + tid] = waves4_sum(&red[0][tid], kSums);
}

// grid F, one wave: the ordered pass over the pair's partials, the 3 x 3 solve, Rodrigues and the scale update in f64
__global__ __launch_bounds__(64) void stab_fit_finish_kernel(const double* __restrict__ partials, int nblk, double* __restrict__ state,
                                                             float* __restrict__ R_out, double* __restrict__ diag, int first,
                                                             double c_min, double px_per_rad) {
    const int pair = blockIdx.x, lane = threadIdx.x;
    const double* P = partials + (size_t)pair * nblk * kPartial;
    double acc[kSums];
#pragma unroll
    for (int k = 0; k < kSums; ++k) acc[k] = 0.0;
    for (int b = lane; b < nblk; b += 64) {
#pragma unroll
        for (int k = 0; k < kSums; ++k) acc[k] += P[(size_t)b * kPartial + k];
    }
#pragma unroll
    for (int k = 0; k < kSums; ++k) acc[k] = wave_sum_down(acc[k]);
    if (lane != 0) return;
    const double Nxx = acc[0], Nxy = acc[1], Nxz = acc[2], Nyy = acc[3], Nyz = acc[4], Nzz = acc[5];
    const double bx = acc[6], by = acc[7], bz = acc[8], sw = acc[9], swr2 = acc[10];
    double* S = state + (size_t)pair * kState;
    float* Ro = R_out + (size_t)pair * 9;
    double* D = diag + (size_t)pair * 4;
    // cofactors of the symmetric N
    const double c00 = Nyy * Nzz - Nyz * Nyz, c01 = Nxz * Nyz - Nxy * Nzz, c02 = Nxy * Nyz - Nxz * Nyy;
    const double c11 = Nxx * Nzz - Nxz * Nxz, c12 = Nxy * Nxz - Nxx * Nyz, c22 = Nxx * Nyy - Nxy * Nxy;
    const double det = Nxx * c00 + Nxy * c01 + Nxz * c02;
    const double tr3 = (Nxx + Nyy + Nzz) / 3.0;
    const bool ok = S[10] == 0.0 && sw > 0.0 && isfinite(det) && det > 1e-12 * tr3 * tr3 * tr3;
    if (!ok) {                                                         // singular: R = I, sum_w = 0, and it stays so
        S[0] = 1.0; S[1] = 0.0; S[2] = 0.0;
        S[3] = 0.0; S[4] = 1.0; S[5] = 0.0;
        S[6] = 0.0; S[7] = 0.0; S[8] = 1.0;
        S[10] = 1.0;
        Ro[0] = 1.f; Ro[1] = 0.f; Ro[2] = 0.f;
        Ro[3] = 0.f; Ro[4] = 1.f; Ro[5] = 0.f;
        Ro[6] = 0.f; Ro[7] = 0.f; Ro[8] = 1.f;
        D[0] = S[9] * px_per_rad;
        D[1] = 0.0;
        D[2] = 0.0;
        D[3] = 0.0;
        return;
    }
    const double dx = (c00 * bx + c01 * by + c02 * bz) / det;
    const double dy = (c01 * bx + c11 * by + c12 * bz) / det;
    const double dz = (c02 * bx + c12 * by + c22 * bz) / det;
    const double t2 = dx * dx + dy * dy + dz * dz;
    const double t = sqrt(t2);
    double A, B;                                                       // sin t / t and (1 - cos t) / t^2
    if (t < 1e-8) {
        A = 1.0 - t2 / 6.0;
        B = 0.5 - t2 / 24.0;
    } else {
        const double sh = sin(0.5 * t);
        A = sin(t) / t;
        B = 2.0 * sh * sh / t2;
    }
    const double e00 = 1.0 + B * (dx * dx - t2), e01 = B * dx * dy - A * dz, e02 = B * dx * dz + A * dy;
    const double e10 = B * dx * dy + A * dz, e11 = 1.0 + B * (dy * dy - t2), e12 = B * dy * dz - A * dx;
    const double e20 = B * dx * dz - A * dy, e21 = B * dy * dz + A * dx, e22 = 1.0 + B * (dz * dz - t2);
    const double r00 = S[0], r01 = S[1], r02 = S[2], r10 = S[3], r11 = S[4], r12 = S[5], r20 = S[6], r21 = S[7], r22 = S[8];
    const double n00 = e00 * r00 + e01 * r10 + e02 * r20, n01 = e00 * r01 + e01 * r11 + e02 * r21, n02 = e00 * r02 + e01 * r12 + e02 * r22;
    const double n10 = e10 * r00 + e11 * r10 + e12 * r20, n11 = e10 * r01 + e11 * r11 + e12 * r21, n12 = e10 * r02 + e11 * r12 + e12 * r22;
    const double n20 = e20 * r00 + e21 * r10 + e22 * r20, n21 = e20 * r01 + e21 * r11 + e22 * r21, n22 = e20 * r02 + e21 * r12 + e22 * r22;
    S[0] = n00; S[1] = n01; S[2] = n02;
    S[3] = n10; S[4] = n11; S[5] = n12;
    S[6] = n20; S[7] = n21; S[8] = n22;
    Ro[0] = (float)n00; Ro[1] = (float)n01; Ro[2] = (float)n02;
    Ro[3] = (float)n10; Ro[4] = (float)n11; Ro[5] = (float)n12;
    Ro[6] = (float)n20; Ro[7] = (float)n21; Ro[8] = (float)n22;
    const double s = sqrt(swr2 / sw);
    const double c = first ? fmax(c_min, 2.0 * s) : fmax(c_min, 0.5 * S[9]);
    S[9] = c;
    S[11] = 1.0 / (c * c);
    D[0] = c * px_per_rad;
    D[1] = sw;
    D[2] = s * px_per_rad;
    D[3] = t;
}

// ------------------------------------------------------------------ K11b: the flow of a rotation
// grid (ceil(W / 256), H, F)
__global__ __launch_bounds__(256) void stab_flow_kernel(const float* __restrict__ Rs, const float2* __restrict__ tabx,
                                                        const float2* __restrict__ taby, float2* __restrict__ G, int H, int W) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const Rot R = load_rot(Rs + (size_t)blockIdx.z * 9);
    float px, py, pz, qx, qy, qz, sx, sy;
    stab_dir(tabx[x], taby[y], px, py, pz);
    stab_rotate(R, px, py, pz, qx, qy, qz);
    stab_pix(qx, qy, qz, 0.5f * (float)W, 0.5f * (float)H, sx, sy);
    float gx = sx - (float)x;
    const float gy = sy - (float)y;
    const float half_w = 0.5f * (float)W;
    if (gx >= half_w) gx -= (float)W;
    if (gx < -half_w) gx += (float)W;
    G[((size_t)blockIdx.z * H + y) * W + x] = make_float2(gx, gy);
}

// ------------------------------------------------------------------ K11c: the frame under a rotation
// grid (ceil(W / 256), H, N): one thread per output pixel, all C channels; wrap in x, clamp in y
template <typename T, int C>
__global__ __launch_bounds__(256) void stab_rotate_kernel(const T* __restrict__ src, const float* __restrict__ Rs,
                                                          const float2* __restrict__ tabx, const float2* __restrict__ taby,
                                                          T* __restrict__ dst, int H, int W) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const Rot R = load_rot(Rs + (size_t)blockIdx.z * 9);
    float px, py, pz, qx, qy, qz, sx, sy;
    stab_dir(tabx[x], taby[y], px, py, pz);
    stab_rotate(R, px, py, pz, qx, qy, qz);
    stab_pix(qx, qy, qz, 0.5f * (float)W, 0.5f * (float)H, sx, sy);
    sphere_sample<T, C>(src + (size_t)blockIdx.z * H * W * C, H, W, sx, sy, dst + (((size_t)blockIdx.z * H + y) * W + x) * C);
}

// ------------------------------------------------------------------ host side
struct WorkLayout {
    size_t state, partials, total;               // byte offsets, behind sphere.h's tables
    int nblk;
};

WorkLayout work_layout(int F, int H, int W) {
    WorkLayout l;
    l.nblk = (int)(((long long)H * W + kFitBlock - 1) / kFitBlock);
    l.state = tab_bytes(H, W);
    l.partials = l.state + (size_t)F * kState * sizeof(double);
    l.total = l.partials + (size_t)F * l.nblk * kPartial * sizeof(double);
    return l;
}

template <typename T, int C>
int launch_rotate(const void* frames, const float* R, const float2* tabx, const float2* taby, void* out, int N, int H, int W,
                  hipStream_t s) {
    hipLaunchKernelGGL((stab_rotate_kernel<T, C>), dim3((W + 255) / 256, H, N), dim3(256), 0, s, (const T*)frames, R, tabx, taby,
                       (T*)out, H, W);
    CP360_CHECK_HIP();
    return CP360_OK;
}

}  // namespace

// ------------------------------------------------------------------ C ABI
extern "C" size_t cp360_stab_work_bytes(int F, int H, int W) {
    if (F < 0 || H <= 0 || W <= 0 || big_image(F > 0 ? F : 1, H, W)) return 0;
    return work_layout(F, H, W).total;
}

extern "C" int cp360_stab_fit(const float* flow, int F, int H, int W, int iters, double c_min_px, float* R, double* diag,
                              void* work, size_t work_bytes, void* stream) {
    if (!flow || !R || !diag || !work) return CP360_ERR_NULL;
    if (bad_image(F, H, W) || iters < 1 || !(c_min_px > 0.0) || !isfinite(c_min_px)) return CP360_ERR_BAD_SHAPE;
    if (big_image(F, H, W)) return CP360_ERR_UNSUPPORTED;
    if (((uintptr_t)flow & 7) != 0) return CP360_ERR_ALIGN;                // read as float2
    const WorkLayout l = work_layout(F, H, W);
    hipStream_t s = (hipStream_t)stream;
    SphereTabs t;
    const int st = open_tabs(work, work_bytes, l.total, H, W, s, &t);
    if (st != CP360_OK) return st;
    double* state = (double*)((char*)work + l.state);
    double* partials = (double*)((char*)work + l.partials);
    const double two_pi = 6.283185307179586476925;
    const double c_min = c_min_px * two_pi / (double)W;
    hipLaunchKernelGGL(stab_fit_init_kernel, dim3((F + 63) / 64), dim3(64), 0, s, state, F, c_min);
    CP360_CHECK_HIP();
    const float kx = (float)(two_pi / (double)W), ky = (float)(0.5 * two_pi / (double)H);
    for (int k = 0; k < iters; ++k) {
        hipLaunchKernelGGL(stab_fit_accum_kernel, dim3(l.nblk, F), dim3(256), 0, s, (const float2*)flow, t.x, t.y,
                           (const double*)state, partials, H, W, kx, ky, k == 0 ? 1 : 0);
        CP360_CHECK_HIP();
        hipLaunchKernelGGL(stab_fit_finish_kernel, dim3(F), dim3(64), 0, s, (const double*)partials, l.nblk, state, R, diag,
                           k == 0 ? 1 : 0, c_min, (double)W / two_pi);
        CP360_CHECK_HIP();
    }
    return CP360_OK;
}

extern "C" int cp360_stab_flow(const float* R, int F, int H, int W, float* G, void* work, size_t work_bytes, void* stream) {
    if (!R || !G || !work) return CP360_ERR_NULL;
    if (bad_image(F, H, W)) return CP360_ERR_BAD_SHAPE;
    if (big_image(F, H, W)) return CP360_ERR_UNSUPPORTED;
    if (((uintptr_t)G & 7) != 0) return CP360_ERR_ALIGN;                   // written as float2
    hipStream_t s = (hipStream_t)stream;
    SphereTabs t;
    const int st = open_tabs(work, work_bytes, tab_bytes(H, W), H, W, s, &t);
    if (st != CP360_OK) return st;
    hipLaunchKernelGGL(stab_flow_kernel, dim3((W + 255) / 256, H, F), dim3(256), 0, s, R, t.x, t.y, (float2*)G, H, W);
    CP360_CHECK_HIP();
    return CP360_OK;
}

extern "C" int cp360_stab_rotate(int dtype, const void* frames, const float* R, int N, int H, int W, int C, void* out, void* work,
                                 size_t work_bytes, void* stream) {
    if (!frames || !R || !out || !work) return CP360_ERR_NULL;
    if (bad_image(N, H, W) || C < 1) return CP360_ERR_BAD_SHAPE;
    if (dtype != CP360_F32 && dtype != CP360_U8) return CP360_ERR_BAD_DTYPE;
    if (C > 4 || (dtype == CP360_U8 && C != 3) || big_image(N, H, W)) return CP360_ERR_UNSUPPORTED;
    if (frames == out) return CP360_ERR_UNSUPPORTED;                   // a gather: not in place
    hipStream_t s = (hipStream_t)stream;
    SphereTabs t;
    const int st = open_tabs(work, work_bytes, tab_bytes(H, W), H, W, s, &t);
    if (st != CP360_OK) return st;
    return dispatch_pixels(dtype, C, [&](auto px, auto c) {
        return launch_rotate<decltype(px), decltype(c)::value>(frames, R, t.x, t.y, out, N, H, W, s);
    });
}

