// K23: ego-motion of a travelling 360-degree camera from the optical flow K10 computes - the rotation R and the direction of
// translation e of every frame pair (K23a) and the part of the flow that this camera motion and a static scene cannot explain at
// any depth, the independent-motion flow (K23b).  The reference has no counterpart; the specification is the package's own,
// DESIGN.md "K23" (7o), and tests/egomotion_restate.py restates it in float64.  Geometry, tables and the ordered sums are sphere.h's;
// every per-pixel term is f32 with plain operators and contraction off, every sum f64 in a fixed order (K11's rule).
//
// Per pixel: p = dir(x, y), p_f = dir(x + dx, y + dy), a = cos phi, g = R^T p_f, n = p x g.  A static point at depth d has
// g = normalize(p - (|T| / d) e): it moves on the great circle through p and -e, away from +e, at most as far as -e.
//
// K23a, per pair, one pass over the flow per iteration k (state R_k, e_k, c_k; R_0 given, e_0 = 0):
//     weights       k = 0: w = a / (|n|^2 + c_min^2); later w = a / (1 + rho^2 / c_k^2)^2, rho^2 = (n . e_k)^2 / max(1 - (p . e_k)^2, 1e-12)
//     gate          pass 0: share = sum a [g . p <= 0 or |n|^2 > sin^2 t_min] / sum a; share < min_share: e = 0, R = R_0, done
//     translation   M = sum w n n^T, e_k+1 = unit eigenvector of its smallest eigenvalue (8 cyclic Jacobi sweeps in f64, scalars
//                   only), signed such that (sum w (g - p)) . e <= 0
//     rotation      k >= 1, with e_k: r = n . e, J = (p . g) e - (e . g) p, A = sum w J J^T, b = sum w r J, d = A^-1 b by cofactors,
//                   R_k+1 = R_k exp([d]x) (the Gauss-Newton step of the epipolar residual written in frame t's axes)
//     scale         c_1 = 4 c_min, c_2 = max(c_min, 2 s) with s the weighted RMS of rho in pass 1, then c_k+1 = max(c_min, c_k / 2)
// Two launches per iteration for all pairs, as K11a: 256 threads x 8 pixels give one f64 partial of 22 sums per workgroup; one
// wave per pair adds the partials in order, solves and updates the pair's state.  No atomics, no host synchronisation, results
// independent of the batch size and of the pair's place in it.
#pragma clang fp contract(off)

#include "sphere.h"

namespace {

constexpr int kFitPx = 8;                    // pixels per thread of the accumulation
constexpr int kFitBlock = 256 * kFitPx;      // pixels per workgroup = per partial
constexpr int kSums = 22;                    // M (6), sum w (g - p) (3), A (6), b (3), sum w, sum w rho^2, sum a, sum a [far]
constexpr int kPartial = 24;                 // doubles per partial (padded)
constexpr int kState = 32;                   // doubles per pair: R[9], e[3], c, 1 / c^2, flag, share
constexpr int kSweeps = 8;                   // cyclic Jacobi sweeps of the 3 x 3 eigen-solve

// direction of (x + dx, y + dy): the angle sums theta + dx 2 pi / W and phi - dy pi / H (stabilize.hip's stab_dir_moved)
__device__ __forceinline__ void ego_dir_moved(const float2 cs_theta, const float2 cs_phi, float dx, float dy, float kx, float ky,
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

// g = R^T p_f
__device__ __forceinline__ void ego_derotate(const Rot& R, float fx, float fy, float fz, float& gx, float& gy, float& gz) {
    gx = R.r00 * fx + R.r10 * fy + R.r20 * fz;
    gy = R.r01 * fx + R.r11 * fy + R.r21 * fz;
    gz = R.r02 * fx + R.r12 * fy + R.r22 * fz;
}

// ------------------------------------------------------------------ K23a: fit
__global__ __launch_bounds__(64) void ego_fit_init_kernel(const float* __restrict__ R0, double* __restrict__ state, int F,
                                                          double c_min) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= F) return;
    double* S = state + (size_t)p * kState;
    const float* r = R0 + (size_t)p * 9;
#pragma unroll
    for (int i = 0; i < 9; ++i) S[i] = (double)r[i];
    S[9] = 0.0; S[10] = 0.0; S[11] = 0.0;
    S[12] = c_min;
    S[13] = 1.0 / (c_min * c_min);
    S[14] = 0.0;
    S[15] = 0.0;
}

// grid (ceil(H W / 2048), F): one partial of 22 f64 sums per workgroup
__global__ __launch_bounds__(256) void ego_fit_accum_kernel(const float2* __restrict__ flow, const float2* __restrict__ tabx,
                                                            const float2* __restrict__ taby, const double* __restrict__ state,
                                                            double* __restrict__ partials, int H, int W, float kx, float ky,
                                                            float cmin2, float sin2t, int first) {
    __shared__ double red[4][kSums];
    const int pair = blockIdx.y, tid = threadIdx.x;
    const int n = H * W;
    const double* S = state + (size_t)pair * kState;
    if (S[14] != 0.0) return;                                              // gated or singular: the pair is done
    Rot R;
    R.r00 = (float)S[0]; R.r01 = (float)S[1]; R.r02 = (float)S[2];
    R.r10 = (float)S[3]; R.r11 = (float)S[4]; R.r12 = (float)S[5];
    R.r20 = (float)S[6]; R.r21 = (float)S[7]; R.r22 = (float)S[8];
    const float ex = (float)S[9], ey = (float)S[10], ez = (float)S[11];
    const float inv_c2 = (float)S[13];
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
        float px, py, pz, fx, fy, fz, gx, gy, gz;
        stab_dir(cst, csp, px, py, pz);
        ego_dir_moved(cst, csp, f.x, f.y, kx, ky, fx, fy, fz);
        ego_derotate(R, fx, fy, fz, gx, gy, gz);
        const float nx = py * gz - pz * gy, ny = pz * gx - px * gz, nz = px * gy - py * gx;
        const float n2 = nx * nx + ny * ny + nz * nz;
        const float gp = px * gx + py * gy + pz * gz;
        const float a = csp.x;
        float w;
        if (first) {
            w = a / (n2 + cmin2);
            acc[20] += (double)a;
            acc[21] += (double)((gp <= 0.f || n2 > sin2t) ? a : 0.f);
        } else {
            const float ne = nx * ex + ny * ey + nz * ez;
            const float pe = px * ex + py * ey + pz * ez;
            const float rho2 = (ne * ne) / fmaxf(1.f - pe * pe, 1e-12f);
            const float u = 1.f + rho2 * inv_c2;
            w = a / (u * u);
            const float ge = gx * ex + gy * ey + gz * ez;
            const float jx = gp * ex - ge * px, jy = gp * ey - ge * py, jz = gp * ez - ge * pz;
            const float wjx = w * jx, wjy = w * jy, wjz = w * jz, wr = w * ne;
            acc[9] += (double)(wjx * jx);
            acc[10] += (double)(wjx * jy);
            acc[11] += (double)(wjx * jz);
            acc[12] += (double)(wjy * jy);
            acc[13] += (double)(wjy * jz);
            acc[14] += (double)(wjz * jz);
            acc[15] += (double)(wr * jx);
            acc[16] += (double)(wr * jy);
            acc[17] += (double)(wr * jz);
            acc[19] += (double)(w * rho2);
        }
        const float wnx = w * nx, wny = w * ny, wnz = w * nz;
        acc[0] += (double)(wnx * nx);
        acc[1] += (double)(wnx * ny);
        acc[2] += (double)(wnx * nz);
        acc[3] += (double)(wny * ny);
        acc[4] += (double)(wny * nz);
        acc[5] += (double)(wnz * nz);
        acc[6] += (double)(w * (gx - px));
        acc[7] += (double)(w * (gy - py));
        acc[8] += (double)(w * (gz - pz));
        acc[18] += (double)w;
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

// one Jacobi rotation that zeroes a_pq of a symmetric 3 x 3 matrix (r is the third index); the columns p and q of V turn with it
__device__ __forceinline__ void ego_jrot(double& app, double& aqq, double& apq, double& apr, double& aqr, double& v0p, double& v0q,
                                         double& v1p, double& v1q, double& v2p, double& v2q) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
    if (theta < 0.0) t = -t;
    const double c = 1.0 / sqrt(t * t + 1.0);
    const double s = t * c;
    app = app - t * apq;
    aqq = aqq + t * apq;
    apq = 0.0;
    const double pr = c * apr - s * aqr, qr = s * apr + c * aqr;
    apr = pr;
    aqr = qr;
    const double n0p = c * v0p - s * v0q, n0q = s * v0p + c * v0q;
    const double n1p = c * v1p - s * v1q, n1q = s * v1p + c * v1q;
    const double n2p = c * v2p - s * v2q, n2q = s * v2p + c * v2q;
    v0p = n0p; v0q = n0q;
    v1p = n1p; v1q = n1q;
    v2p = n2p; v2q = n2q;
}

// the pair is done: R = R_0, e = 0, and later passes leave it alone
__device__ __forceinline__ void ego_close(double* S, const float* R0, float* Ro, float* Eo, double* D, double flag, double c_min_px) {
    S[14] = flag;
#pragma unroll
    for (int i = 0; i < 9; ++i) Ro[i] = R0[i];
    Eo[0] = 0.f; Eo[1] = 0.f; Eo[2] = 0.f;
    D[0] = S[15];
    D[1] = 0.0; D[2] = 0.0; D[3] = 0.0; D[4] = 0.0; D[5] = 0.0;
    D[6] = c_min_px;
    D[7] = flag;
}

// grid F, one wave: the ordered pass over the pair's partials, the gate, the eigen-solve, the 3 x 3 solve, Rodrigues and the
// scale update in f64
__global__ __launch_bounds__(64) void ego_fit_finish_kernel(const double* __restrict__ partials, int nblk, double* __restrict__ state,
                                                            const float* __restrict__ R0, float* __restrict__ R_out,
                                                            float* __restrict__ e_out, double* __restrict__ diag, int k,
                                                            double c_min, double min_share, double px_per_rad) {
    const int pair = blockIdx.x, lane = threadIdx.x;
    double* S = state + (size_t)pair * kState;
    if (S[14] != 0.0) return;
    const double* P = partials + (size_t)pair * nblk * kPartial;
    double acc[kSums];
#pragma unroll
    for (int i = 0; i < kSums; ++i) acc[i] = 0.0;
    for (int b = lane; b < nblk; b += 64) {
#pragma unroll
        for (int i = 0; i < kSums; ++i) acc[i] += P[(size_t)b * kPartial + i];
    }
#pragma unroll
    for (int i = 0; i < kSums; ++i) acc[i] = wave_sum_down(acc[i]);
    if (lane != 0) return;
    const float* R0p = R0 + (size_t)pair * 9;
    float* Ro = R_out + (size_t)pair * 9;
    float* Eo = e_out + (size_t)pair * 3;
    double* D = diag + (size_t)pair * 8;
    const double sw = acc[18], swr = acc[19];
    if (k == 0) {                                                          // the gate, at R_0
        const double s_a = acc[20];
        if (!(s_a > 0.0)) {
            S[15] = 0.0;
            ego_close(S, R0p, Ro, Eo, D, 2.0, c_min * px_per_rad);
            return;
        }
        S[15] = acc[21] / s_a;
        if (S[15] < min_share) {
            ego_close(S, R0p, Ro, Eo, D, 1.0, c_min * px_per_rad);
            return;
        }
    }
    // ---- translation: the eigenvector of M's smallest eigenvalue
    double a00 = acc[0], a01 = acc[1], a02 = acc[2], a11 = acc[3], a12 = acc[4], a22 = acc[5];
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
#pragma unroll
    for (int sweep = 0; sweep < kSweeps; ++sweep) {
        ego_jrot(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
        ego_jrot(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
        ego_jrot(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
    }
    // ascending eigenvalues by three compare-exchanges; column 0 of V goes with the smallest (columns 1 and 2 are not needed
    // beyond the exchange that may bring one of them to the front)
    double l0 = a00, l1 = a11, l2 = a22, x0 = v00, y0 = v10, z0 = v20, x1 = v01, y1 = v11, z1 = v21;
    const bool s01 = l1 < l0;
    const double m0 = s01 ? l1 : l0, m1 = s01 ? l0 : l1;
    x0 = s01 ? v01 : v00; y0 = s01 ? v11 : v10; z0 = s01 ? v21 : v20;
    x1 = s01 ? v00 : v01; y1 = s01 ? v10 : v11; z1 = s01 ? v20 : v21;
    const bool s12 = l2 < m1;
    const double m1b = s12 ? l2 : m1, m2 = s12 ? m1 : l2;
    x1 = s12 ? v02 : x1; y1 = s12 ? v12 : y1; z1 = s12 ? v22 : z1;
    const bool s01b = m1b < m0;
    l0 = s01b ? m1b : m0; l1 = s01b ? m0 : m1b; l2 = m2;
    x0 = s01b ? x1 : x0; y0 = s01b ? y1 : y0; z0 = s01b ? z1 : z0;
    if (!(sw > 0.0 && isfinite(l0) && isfinite(l1) && isfinite(l2) && l2 > 0.0 && l1 > 1e-12 * l2)) {
        ego_close(S, R0p, Ro, Eo, D, 2.0, c_min * px_per_rad);
        return;
    }
    const double nrm = sqrt(x0 * x0 + y0 * y0 + z0 * z0);
    x0 = x0 / nrm; y0 = y0 / nrm; z0 = z0 / nrm;
    const double dot = acc[6] * x0 + acc[7] * y0 + acc[8] * z0;
    const double first_nz = x0 != 0.0 ? x0 : (y0 != 0.0 ? y0 : z0);
    if (dot > 0.0 || (dot == 0.0 && first_nz < 0.0)) {
        x0 = -x0; y0 = -y0; z0 = -z0;
    }
    // ---- rotation: Gauss-Newton on the epipolar residual, with the e the pass was weighted by
    double t = 0.0;
    if (k > 0) {
        const double Nxx = acc[9], Nxy = acc[10], Nxz = acc[11], Nyy = acc[12], Nyz = acc[13], Nzz = acc[14];
        const double bx = acc[15], by = acc[16], bz = acc[17];
        const double c00 = Nyy * Nzz - Nyz * Nyz, c01 = Nxz * Nyz - Nxy * Nzz, c02 = Nxy * Nyz - Nxz * Nyy;
        const double c11 = Nxx * Nzz - Nxz * Nxz, c12 = Nxy * Nxz - Nxx * Nyz, c22 = Nxx * Nyy - Nxy * Nxy;
        const double det = Nxx * c00 + Nxy * c01 + Nxz * c02;
        const double tr3 = (Nxx + Nyy + Nzz) / 3.0;
        if (isfinite(det) && det > 1e-12 * tr3 * tr3 * tr3) {
            const double dx = (c00 * bx + c01 * by + c02 * bz) / det;
            const double dy = (c01 * bx + c11 * by + c12 * bz) / det;
            const double dz = (c02 * bx + c12 * by + c22 * bz) / det;
            const double t2 = dx * dx + dy * dy + dz * dz;
            t = sqrt(t2);
            double A, B;                                                   // sin t / t and (1 - cos t) / t^2
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
            S[0] = r00 * e00 + r01 * e10 + r02 * e20; S[1] = r00 * e01 + r01 * e11 + r02 * e21; S[2] = r00 * e02 + r01 * e12 + r02 * e22;
            S[3] = r10 * e00 + r11 * e10 + r12 * e20; S[4] = r10 * e01 + r11 * e11 + r12 * e21; S[5] = r10 * e02 + r11 * e12 + r12 * e22;
            S[6] = r20 * e00 + r21 * e10 + r22 * e20; S[7] = r20 * e01 + r21 * e11 + r22 * e21; S[8] = r20 * e02 + r21 * e12 + r22 * e22;
        }
    }
    const double s = sqrt(swr / sw);
    const double c = k == 0 ? 4.0 * c_min : (k == 1 ? fmax(c_min, 2.0 * s) : fmax(c_min, 0.5 * S[12]));
    S[9] = x0; S[10] = y0; S[11] = z0;
    S[12] = c;
    S[13] = 1.0 / (c * c);
#pragma unroll
    for (int i = 0; i < 9; ++i) Ro[i] = (float)S[i];
    Eo[0] = (float)x0; Eo[1] = (float)y0; Eo[2] = (float)z0;
    D[0] = S[15];
    D[1] = sw;
    D[2] = s * px_per_rad;
    D[3] = l0 / l2;
    D[4] = l1 / l2;
    D[5] = t;
    D[6] = c * px_per_rad;
    D[7] = 0.0;
}

// ------------------------------------------------------------------ K23b: the independent-motion flow
// grid (ceil(W / 256), H, F): one thread per pixel
__global__ __launch_bounds__(256) void ego_residual_kernel(const float2* __restrict__ flow, const float* __restrict__ Rs,
                                                           const float* __restrict__ es, const float2* __restrict__ tabx,
                                                           const float2* __restrict__ taby, float2* __restrict__ res,
                                                           float* __restrict__ mag, int H, int W, float kx, float ky,
                                                           float px_per_rad) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const size_t i = ((size_t)blockIdx.z * H + y) * W + x;
    const float2 f = flow[i];
    if (!(isfinite(f.x) && isfinite(f.y))) {
        res[i] = make_float2(NAN, NAN);
        if (mag) mag[i] = NAN;
        return;
    }
    const Rot R = load_rot(Rs + (size_t)blockIdx.z * 9);
    const float ex = es[(size_t)blockIdx.z * 3], ey = es[(size_t)blockIdx.z * 3 + 1], ez = es[(size_t)blockIdx.z * 3 + 2];
    const float2 cst = tabx[x], csp = taby[y];
    float px, py, pz, fx, fy, fz, gx, gy, gz;
    stab_dir(cst, csp, px, py, pz);
    ego_dir_moved(cst, csp, f.x, f.y, kx, ky, fx, fy, fz);
    ego_derotate(R, fx, fy, fz, gx, gy, gz);
    float sx = px, sy = py, sz = pz;                                       // g*: e = 0 explains no motion at all
    if (ex != 0.f || ey != 0.f || ez != 0.f) {
        const float pe = px * ex + py * ey + pz * ez;
        const float kx2 = py * ez - pz * ey, ky2 = pz * ex - px * ez, kz2 = px * ey - py * ex;
        const float s2 = kx2 * kx2 + ky2 * ky2 + kz2 * kz2;               // 1 - (p . e)^2 as |p x e|^2: f32 resolves it at an epipole
        if (s2 < 1e-12f) {                                                 // an epipole: every motion is epipolar
            sx = gx; sy = gy; sz = gz;
        } else {
            const float rs = sqrtf(s2);
            const float ux = (pe * px - ex) / rs, uy = (pe * py - ey) / rs, uz = (pe * pz - ez) / rs;
            float al = atan2f(gx * ux + gy * uy + gz * uz, gx * px + gy * py + gz * pz);
            al = fminf(fmaxf(al, 0.f), atan2f(rs, -pe));
            float sa, ca;
            sincosf(al, &sa, &ca);
            sx = ca * px + sa * ux;
            sy = ca * py + sa * uy;
            sz = ca * pz + sa * uz;
        }
    }
    const float half_w = 0.5f * (float)W, half_h = 0.5f * (float)H;
    float x1, y1, x0, y0;
    stab_pix(gx, gy, gz, half_w, half_h, x1, y1);
    stab_pix(sx, sy, sz, half_w, half_h, x0, y0);
    float rx = x1 - x0;
    if (rx >= half_w) rx -= (float)W;
    if (rx < -half_w) rx += (float)W;
    res[i] = make_float2(rx, y1 - y0);
    if (mag) {
        const float cx = gy * sz - gz * sy, cy = gz * sx - gx * sz, cz = gx * sy - gy * sx;
        mag[i] = atan2f(sqrtf(cx * cx + cy * cy + cz * cz), gx * sx + gy * sy + gz * sz) * px_per_rad;
    }
}

// ------------------------------------------------------------------ host side
struct EgoLayout {
    size_t state, partials, total;               // byte offsets, behind sphere.h's tables
    int nblk;
};

EgoLayout ego_layout(int F, int H, int W) {
    EgoLayout l;
    l.nblk = (int)(((long long)H * W + kFitBlock - 1) / kFitBlock);
    l.state = tab_bytes(H, W);
    l.partials = l.state + (size_t)F * kState * sizeof(double);
    l.total = l.partials + (size_t)F * l.nblk * kPartial * sizeof(double);
    return l;
}

}  // namespace

// ------------------------------------------------------------------ C ABI
extern "C" size_t cp360_ego_work_bytes(int F, int H, int W) {
    if (F < 0 || H <= 0 || W <= 0 || big_image(F > 0 ? F : 1, H, W)) return 0;
    return ego_layout(F, H, W).total;
}

extern "C" int cp360_ego_fit(const float* flow, const float* R0, int F, int H, int W, int iters, double c_min_px, double t_min_px,
                             double min_share, float* R, float* e, double* diag, void* work, size_t work_bytes, void* stream) {
    if (!flow || !R0 || !R || !e || !diag || !work) return CP360_ERR_NULL;
    if (bad_image(F, H, W) || iters < 1 || !(c_min_px > 0.0) || !isfinite(c_min_px) || !(t_min_px >= 0.0) || !isfinite(t_min_px) ||
        !(min_share >= 0.0) || !isfinite(min_share))
        return CP360_ERR_BAD_SHAPE;
    if (big_image(F, H, W)) return CP360_ERR_UNSUPPORTED;
    if (((uintptr_t)flow & 7) != 0) return CP360_ERR_ALIGN;                // read as float2
    const EgoLayout l = ego_layout(F, H, W);
    hipStream_t s = (hipStream_t)stream;
    SphereTabs t;
    const int st = open_tabs(work, work_bytes, l.total, H, W, s, &t);
    if (st != CP360_OK) return st;
    double* state = (double*)((char*)work + l.state);
    double* partials = (double*)((char*)work + l.partials);
    const double two_pi = 6.283185307179586476925;
    const double c_min = c_min_px * two_pi / (double)W;
    const double t_min = fmin(t_min_px * two_pi / (double)W, 0.25 * two_pi);
    const double sin_t = sin(t_min);
    hipLaunchKernelGGL(ego_fit_init_kernel, dim3((F + 63) / 64), dim3(64), 0, s, R0, state, F, c_min);
    CP360_CHECK_HIP();
    const float kx = (float)(two_pi / (double)W), ky = (float)(0.5 * two_pi / (double)H);
    for (int k = 0; k < iters; ++k) {
        hipLaunchKernelGGL(ego_fit_accum_kernel, dim3(l.nblk, F), dim3(256), 0, s, (const float2*)flow, t.x, t.y,
                           (const double*)state, partials, H, W, kx, ky, (float)(c_min * c_min), (float)(sin_t * sin_t),
                           k == 0 ? 1 : 0);
        CP360_CHECK_HIP();
        hipLaunchKernelGGL(ego_fit_finish_kernel, dim3(F), dim3(64), 0, s, (const double*)partials, l.nblk, state, R0, R, e, diag,
                           k < 2 ? k : 2, c_min, min_share, (double)W / two_pi);
        CP360_CHECK_HIP();
    }
    return CP360_OK;
}

extern "C" int cp360_ego_residual(const float* flow, const float* R, const float* e, int F, int H, int W, float* res, float* mag,
                                  void* work, size_t work_bytes, void* stream) {
    if (!flow || !R || !e || !res || !work) return CP360_ERR_NULL;         // mag may be null: not wanted
    if (bad_image(F, H, W)) return CP360_ERR_BAD_SHAPE;
    if (big_image(F, H, W)) return CP360_ERR_UNSUPPORTED;
    if ((((uintptr_t)flow | (uintptr_t)res) & 7) != 0) return CP360_ERR_ALIGN;     // read and written as float2
    hipStream_t s = (hipStream_t)stream;
    SphereTabs t;
    const int st = open_tabs(work, work_bytes, tab_bytes(H, W), H, W, s, &t);
    if (st != CP360_OK) return st;
    const double two_pi = 6.283185307179586476925;
    hipLaunchKernelGGL(ego_residual_kernel, dim3((W + 255) / 256, H, F), dim3(256), 0, s, (const float2*)flow, R, e, t.x, t.y,
                       (float2*)res, mag, H, W, (float)(two_pi / (double)W), (float)(0.5 * two_pi / (double)H),
                       (float)((double)W / two_pi));
    CP360_CHECK_HIP();
    return CP360_OK;
}
