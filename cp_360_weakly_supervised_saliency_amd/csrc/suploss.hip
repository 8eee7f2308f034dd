// K18: the supervised loss - K14's KL, CC and NSS of N saliency maps against N ground-truth maps on the h x w evaluation grid,
// with the gradient with respect to the maps.  The forward pass is sphere_eval.hip's K14a without the ROC (same resampler, same
// passes, same fixed-tree sums: at kl_eps = 2^-52 the three terms are K14's); the specification is DESIGN.md "K18" and
// tests/suploss_restate.py restates it in float64.
//
//   S = cp360_seval_resample(m);  a_i, A, sum_a, mu, M as in sphere_eval.hip;  s = S - mu_S, g = G - mu_G, Vs = sum_a s^2,
//   Vg = sum_a g^2, sigma = sqrt(Vs / A), n = |M|, Z = sum_a (S - min S), P_i = a_i (S_i - min S) / Z, Q alike from G
//   dCC/dS_j  = a_j (g_j / sqrt(Vs Vg) - CC s_j / Vs)
//   dNSS/dS_j = ([j in M] / n - a_j / A) / sigma - NSS a_j s_j / (A sigma^2)
//   dKL/dS_j  = a_j (k_j - K1) / Z for j != mm,  ((A - a_mm) K1 - K2) / Z for j = mm;  r_i = Q_i / (P_i + eps),
//               k_i = -Q_i r_i / ((P_i + eps)(eps + r_i)),  mm = the lowest index with S_mm = min S,
//               K1 = sum_{i != mm} k_i P_i,  K2 = sum_{i != mm} k_i a_i  (P_mm is 0 identically: k_mm, of the order Q_mm / eps,
//               stays out of the sums instead of being cancelled afterwards)
//   dm = the adjoint of the resampler applied to dS = sum_t gterms_t valid_t dterm_t/dS
//
// Launches, all on the caller's stream, no host synchronisation, no atomics:
//   forward   the resampler, then K18a: one 1024-thread workgroup per map, three passes over the map through L2 (sums and minima;
//             centred sums, masses and mm; KL, NSS, the mask's count, K1, K2), reduced by roc_reduce's fixed tree -> terms, valid and
//             the 16 scalars of `stats` the backward pass needs
//   backward  the resampler again (S is recomputed, not kept), K18b: one thread per grid pixel recomputes its P, Q, k from `stats`
//             and writes dS in f64 to the workspace, K18c: one thread per pixel of the small map gathers the grid pixels whose
//             taps reach it, in ascending (row, column) order, the tap weight (column factor x row factor) formed in double from
//             the sampler's f32 fractions, and rounds the f64 sum to f32 once
#include "roc.h"

#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int kSupThreads = kRocThreads;     // K18a
constexpr int kSupWaves = kRocWaves;
constexpr int kSupMaxWeight = 1024;          // K14's clamp
constexpr int kStats = CP360_SUP_LOSS_STATS;
// stats f64 [N, 16]
enum { ST_MU_S, ST_MU_G, ST_VS, ST_VG, ST_MIN_S, ST_MIN_G, ST_Z, ST_ZG, ST_K1, ST_K2, ST_MM, ST_N, ST_A, ST_THR, ST_CC, ST_NSS };
static_assert(ST_NSS + 1 == kStats, "the header's count");

struct SupLayout {
    size_t s, ds, total;
};

SupLayout sup_layout(int N, int P) {
    SupLayout l;
    const size_t n = (size_t)N * (size_t)P;
    l.s = 0;
    l.ds = align16(n * sizeof(float));
    l.total = l.ds + align16(n * sizeof(double));
    return l;
}

struct SupMinF { __device__ float operator()(float a, float b) const { return fminf(a, b); } };
struct SupMinI { __device__ int operator()(int a, int b) const { return a < b ? a : b; } };

__device__ __forceinline__ int sup_weight(const int* __restrict__ wrow, int y) {
    const int a = wrow[y];
    return a < 0 ? 0 : (a > kSupMaxWeight ? kSupMaxWeight : a);
}

// k_i of the KL's gradient from P_i and Q_i
__device__ __forceinline__ double sup_k(double p, double q, double eps) {
    const double pe = p + eps;
    const double r = q / pe;
    return -(q * r) / (pe * (eps + r));
}

// ------------------------------------------------------------------ K18a: the three terms and the scalars of the gradient
// grid N, 1024 threads
__global__ __launch_bounds__(kSupThreads) void sup_forward_kernel(const float* __restrict__ S, const float* __restrict__ G,
                                                                  const uint8_t* __restrict__ fix, const int* __restrict__ wrow,
                                                                  int h, int w, double eps, double* __restrict__ terms,
                                                                  uint8_t* __restrict__ valid, double* __restrict__ stats) {
    __shared__ double smd[kSupWaves * 5];
    __shared__ long long sml[kSupWaves * 3];
    __shared__ float smf[kSupWaves * 2];
    __shared__ int smi[kSupWaves];
    const int tid = threadIdx.x, f = blockIdx.x, P = h * w;
    S += (size_t)f * P;
    G += (size_t)f * P;
    if (fix) fix += (size_t)f * P;
    // pass 1: weighted sums, minima, A, and whether every value is finite (K14a's pass 1)
    double s1[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    float mn[2] = {INFINITY, INFINITY};
    long long ia[3] = {0, 0, 0};
    for (int i = tid; i < P; i += kSupThreads) {
        const int a = sup_weight(wrow, i / w);
        const float s = S[i], g = G[i];
        s1[0] += (double)a * (double)s;
        s1[1] += (double)a * (double)g;
        mn[0] = fminf(mn[0], s);
        mn[1] = fminf(mn[1], g);
        ia[0] += a;
        ia[1] += !(fabsf(s) < INFINITY) || !(fabsf(g) < INFINITY);
    }
    roc_reduce(s1, smd, RocAdd());
    roc_reduce(mn, smf, SupMinF());
    roc_reduce(ia, sml, RocAdd());
    const double A = (double)ia[0];
    const bool bad = ia[1] != 0;
    const double mu_s = s1[0] / A, mu_g = s1[1] / A;
    const double min_s = (double)mn[0], min_g = (double)mn[1];
    // pass 2: centred sums, the masses above the minima, and the lowest index that holds the minimum of S
    double s2[5] = {0.0, 0.0, 0.0, 0.0, 0.0};                          // Vs, Vg, Csg, Z, Zg
    int im[1] = {P};
    for (int i = tid; i < P; i += kSupThreads) {
        const double a = (double)sup_weight(wrow, i / w);
        const float sf = S[i];
        const double s = (double)sf, g = (double)G[i];
        const double ds = s - mu_s, dg = g - mu_g;
        s2[0] += a * (ds * ds);
        s2[1] += a * (dg * dg);
        s2[2] += a * (ds * dg);
        s2[3] += a * (s - min_s);
        s2[4] += a * (g - min_g);
        if (sf == mn[0] && i < im[0]) im[0] = i;
    }
    roc_reduce(s2, smd, RocAdd());
    roc_reduce(im, smi, SupMinI());
    const int mm = im[0];                                              // P when the map holds a NaN: such a map is invalid
    const double sig_s = sqrt(s2[0] / A), sig_g = sqrt(s2[1] / A);
    const double thr = mu_g + 2.0 * sig_g;
    const double mass_s = s2[3], mass_g = s2[4];
    // pass 3: KL, NSS, the mask's count, K1 and K2
    double s3[5] = {0.0, 0.0, 0.0, 0.0, 0.0};                          // KL, NSS sum, K1, K2
    long long i3[3] = {0, 0, 0};                                       // n_fix
    for (int i = tid; i < P; i += kSupThreads) {
        const double a = (double)sup_weight(wrow, i / w);
        const double s = (double)S[i], g = (double)G[i];
        const bool fx = fix ? fix[i] != 0 : g > thr;
        const double p = a * (s - min_s) / mass_s, q = a * (g - min_g) / mass_g;
        s3[0] += q * log(eps + q / (p + eps));
        if (fx) s3[1] += (s - mu_s) / sig_s;
        i3[0] += fx;
        if (i != mm) {
            const double k = sup_k(p, q, eps);
            s3[2] += k * p;
            s3[3] += k * a;
        }
    }
    roc_reduce(s3, smd, RocAdd());
    roc_reduce(i3, sml, RocAdd());
    if (tid == 0) {
        const int n_fix = (int)i3[0];
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        const bool mass = mass_s > 0.0 && mass_g > 0.0;                // zero mass: 0 / 0
        const double kl = bad || !mass ? nan : s3[0];
        const double cc = bad ? nan : s2[2] / sqrt(s2[0] * s2[1]);
        const double nss = bad || n_fix == P ? nan : s3[1] / (double)n_fix;
        double* o = terms + (size_t)f * 3;
        o[0] = kl;
        o[1] = cc;
        o[2] = nss;
        uint8_t* v = valid + (size_t)f * 3;
        // a term is used only when it and what its gradient divides by are finite
        v[0] = fabs(kl) < INFINITY && fabs(s3[2]) < INFINITY && fabs(s3[3]) < INFINITY && mm < P;
        v[1] = fabs(cc) < INFINITY && s2[0] > 0.0 && s2[1] > 0.0;
        v[2] = fabs(nss) < INFINITY && s2[0] > 0.0 && n_fix > 0;
        double* st = stats + (size_t)f * kStats;
        st[ST_MU_S] = mu_s;
        st[ST_MU_G] = mu_g;
        st[ST_VS] = s2[0];
        st[ST_VG] = s2[1];
        st[ST_MIN_S] = min_s;
        st[ST_MIN_G] = min_g;
        st[ST_Z] = mass_s;
        st[ST_ZG] = mass_g;
        st[ST_K1] = s3[2];
        st[ST_K2] = s3[3];
        st[ST_MM] = (double)mm;
        st[ST_N] = (double)n_fix;
        st[ST_A] = A;
        st[ST_THR] = thr;
        st[ST_CC] = cc;
        st[ST_NSS] = nss;
    }
}

// ------------------------------------------------------------------ K18b: dS, per grid pixel
// grid (ceil(P / 256), N), 256 threads.  dS f64 [N, P] = sum_t gterms_t valid_t dterm_t/dS; a term that is invalid or whose
// gterms entry is 0 is skipped, not multiplied: it contributes +0 whatever its derivative holds
__global__ __launch_bounds__(256) void sup_ds_kernel(const float* __restrict__ S, const float* __restrict__ G,
                                                     const uint8_t* __restrict__ fix, const int* __restrict__ wrow,
                                                     const double* __restrict__ stats, const uint8_t* __restrict__ valid,
                                                     const double* __restrict__ gterms, int h, int w, double eps,
                                                     double* __restrict__ dS) {
    const int j = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y, P = h * w;
    if (j >= P) return;
    const double* st = stats + (size_t)f * kStats;
    const double gk = gterms[(size_t)f * 3], gc = gterms[(size_t)f * 3 + 1], gn = gterms[(size_t)f * 3 + 2];
    const bool use_kl = valid[(size_t)f * 3] != 0 && gk != 0.0;
    const bool use_cc = valid[(size_t)f * 3 + 1] != 0 && gc != 0.0;
    const bool use_nss = valid[(size_t)f * 3 + 2] != 0 && gn != 0.0;
    double d = 0.0;
    if (use_kl || use_cc || use_nss) {
        const size_t at = (size_t)f * P + j;
        const double a = (double)sup_weight(wrow, j / w);
        const double s = (double)S[at], g = (double)G[at];
        const double A = st[ST_A], Vs = st[ST_VS];
        const double ss = s - st[ST_MU_S];
        if (use_kl) {
            const double Z = st[ST_Z], K1 = st[ST_K1];
            const int mm = (int)st[ST_MM];
            if (j == mm) {
                const double a_mm = (double)sup_weight(wrow, mm / w);
                d += gk * (((A - a_mm) * K1 - st[ST_K2]) / Z);
            } else {
                const double p = a * (s - st[ST_MIN_S]) / Z, q = a * (g - st[ST_MIN_G]) / st[ST_ZG];
                d += gk * (a * (sup_k(p, q, eps) - K1) / Z);
            }
        }
        if (use_cc) d += gc * (a * ((g - st[ST_MU_G]) / sqrt(Vs * st[ST_VG]) - st[ST_CC] * ss / Vs));
        if (use_nss) {
            const double sigma = sqrt(Vs / A);
            const bool fx = fix ? fix[at] != 0 : g > st[ST_THR];
            d += gn * (((fx ? 1.0 / st[ST_N] : 0.0) - a / A) / sigma - st[ST_NSS] * a * ss / (A * (sigma * sigma)));
        }
    }
    dS[(size_t)f * P + j] = d;
}

// ------------------------------------------------------------------ K18c: the adjoint of the resampler, in gather form
// The taps of grid column x (row y alike): sphere_sample's own f32 terms, so that the weights are those the forward pass used
__device__ __forceinline__ void sup_taps_x(int x, int w, int ws, int& x0, int& x1, float& tx) {
    float sx = (float)((double)((long long)(2 * x + 1) * ws) / (double)(2 * w) - 0.5);
    if (!(fabsf(sx) <= (float)ws)) sx = 0.f;
    const float x0f = floorf(sx);
    tx = sx - x0f;
    x0 = (int)x0f % ws;
    if (x0 < 0) x0 += ws;
    x1 = x0 + 1 == ws ? 0 : x0 + 1;
}

__device__ __forceinline__ void sup_taps_y(int y, int h, int hs, int& y0, int& y1, float& ty) {
    float sy = (float)((double)((long long)(2 * y + 1) * hs) / (double)(2 * h) - 0.5);
    sy = fminf(fmaxf(sy, 0.f), (float)(hs - 1));
    const float y0f = floorf(sy);
    ty = sy - y0f;
    y0 = (int)y0f;
    y1 = y0 + 1 < hs ? y0 + 1 : hs - 1;
}

// the grid indices whose unclamped source position lies within one source pixel of k, two indices of margin for the rounding:
// lo may be negative and hi may pass n - 1 (the caller clamps rows and wraps columns)
__device__ __forceinline__ void sup_span(int k, int n, int ns, int& lo, int& hi) {
    const double scale = (double)(2 * (long long)n) / (double)ns;
    lo = (int)floor((((double)k - 0.5) * scale - 1.0) * 0.5) - 2;
    hi = (int)ceil((((double)k + 1.5) * scale - 1.0) * 0.5) + 2;
}

// grid (ceil(hs ws / 256), N), 256 threads: a thread owns one pixel of the small map
__global__ __launch_bounds__(256) void sup_adjoint_kernel(const double* __restrict__ dS, int h, int w, float* __restrict__ dm,
                                                          int hs, int ws) {
    const int k = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
    if (k >= hs * ws) return;
    dS += (size_t)f * h * w;
    dm += (size_t)f * hs * ws;
    if (hs == h && ws == w) {                                          // the resampler copied: so does its adjoint
        dm[k] = (float)dS[k];
        return;
    }
    const int ys = k / ws, xs = k - ys * ws;
    int ylo, yhi, xlo, xhi;
    sup_span(ys, h, hs, ylo, yhi);
    sup_span(xs, w, ws, xlo, xhi);
    if (ylo < 0 || ys == 0) ylo = 0;                                   // rows clamp: the first and the last source row collect
    if (yhi > h - 1 || ys == hs - 1) yhi = h - 1;                      // from every grid row beyond them
    if ((long long)xhi - xlo + 1 >= w) {                               // the span covers the circle: every column once
        xlo = 0;
        xhi = w - 1;
    }
    double acc = 0.0;
    for (int y = ylo; y <= yhi; ++y) {
        int y0, y1;
        float ty;
        sup_taps_y(y, h, hs, y0, y1, ty);
        if (y0 != ys && y1 != ys) continue;
        const double r0 = 1.0 - (double)ty, r1 = (double)ty;
        const double* row = dS + (size_t)y * w;
        for (int xu = xlo; xu <= xhi; ++xu) {
            const int x = ((xu % w) + w) % w;                          // columns wrap
            int x0, x1;
            float tx;
            sup_taps_x(x, w, ws, x0, x1, tx);
            if (x0 != xs && x1 != xs) continue;
            const double c0 = 1.0 - (double)tx, c1 = (double)tx;
            const double d = row[x];
            if (y0 == ys && x0 == xs) acc += (c0 * r0) * d;
            if (y0 == ys && x1 == xs) acc += (c1 * r0) * d;
            if (y1 == ys && x0 == xs) acc += (c0 * r1) * d;
            if (y1 == ys && x1 == xs) acc += (c1 * r1) * d;
        }
    }
    dm[k] = (float)acc;
}

// the checks the two entry points share, before any HIP call
int sup_args(int N, int mh, int mw, int h, int w, double kl_eps) {
    if (bad_image(N, mh, mw) || bad_image(N, h, w)) return CP360_ERR_BAD_SHAPE;
    if (!(kl_eps > 0.0) || !(kl_eps < INFINITY)) return CP360_ERR_BAD_SHAPE;
    const int st = roc_args(N, h, w);
    if (st != CP360_OK) return st;
    if (big_image(N, mh, mw) || (long long)mh * mw > kRocMaxP) return CP360_ERR_UNSUPPORTED;
    return CP360_OK;
}

}  // namespace

// ------------------------------------------------------------------ C ABI
extern "C" size_t cp360_sup_loss_work_bytes(int N, int mh, int mw, int h, int w) {
    if (sup_args(N, mh, mw, h, w, 1.0) != CP360_OK) return 0;
    return sup_layout(N, h * w).total;
}

extern "C" int cp360_sup_loss_forward(const float* maps, const float* G, const uint8_t* fix, const int32_t* weights, int N, int mh,
                                      int mw, int h, int w, double kl_eps, double* terms, uint8_t* valid, double* stats, void* work,
                                      size_t work_bytes, void* stream) {
    if (!maps || !G || !weights || !terms || !valid || !stats || !work) return CP360_ERR_NULL;
    int st = sup_args(N, mh, mw, h, w, kl_eps);
    if (st != CP360_OK) return st;
    if (!aligned16(work) || (((uintptr_t)terms | (uintptr_t)stats) & 7) != 0 ||
        (((uintptr_t)maps | (uintptr_t)G | (uintptr_t)weights) & 3) != 0)
        return CP360_ERR_ALIGN;
    const int P = h * w;
    const SupLayout l = sup_layout(N, P);
    if (work_bytes < l.total) return CP360_ERR_BAD_SHAPE;
    float* S = (float*)((char*)work + l.s);
    hipStream_t s = (hipStream_t)stream;
    st = cp360_seval_resample(maps, N, mh, mw, S, h, w, stream);
    if (st != CP360_OK) return st;
    hipLaunchKernelGGL(sup_forward_kernel, dim3(N), dim3(kSupThreads), 0, s, (const float*)S, G, fix, (const int*)weights, h, w, kl_eps,
                       terms, valid, stats);
    CP360_CHECK_HIP();
    return CP360_OK;
}

extern "C" int cp360_sup_loss_backward(const float* maps, const float* G, const uint8_t* fix, const int32_t* weights,
                                       const double* stats, const uint8_t* valid, const double* gterms, int N, int mh, int mw, int h,
                                       int w, double kl_eps, float* dmaps, void* work, size_t work_bytes, void* stream) {
    if (!maps || !G || !weights || !stats || !valid || !gterms || !dmaps || !work) return CP360_ERR_NULL;
    int st = sup_args(N, mh, mw, h, w, kl_eps);
    if (st != CP360_OK) return st;
    if (!aligned16(work) || (((uintptr_t)stats | (uintptr_t)gterms) & 7) != 0 ||
        (((uintptr_t)maps | (uintptr_t)G | (uintptr_t)weights | (uintptr_t)dmaps) & 3) != 0)
        return CP360_ERR_ALIGN;
    const int P = h * w;
    const SupLayout l = sup_layout(N, P);
    if (work_bytes < l.total) return CP360_ERR_BAD_SHAPE;
    float* S = (float*)((char*)work + l.s);
    double* dS = (double*)((char*)work + l.ds);
    hipStream_t s = (hipStream_t)stream;
    st = cp360_seval_resample(maps, N, mh, mw, S, h, w, stream);
    if (st != CP360_OK) return st;
    hipLaunchKernelGGL(sup_ds_kernel, dim3((P + 255) / 256, N), dim3(256), 0, s, (const float*)S, G, fix, (const int*)weights, stats,
                       valid, gterms, h, w, kl_eps, dS);
    CP360_CHECK_HIP();
    hipLaunchKernelGGL(sup_adjoint_kernel, dim3((mh * mw + 255) / 256, N), dim3(256), 0, s, (const double*)dS, h, w, dmaps, mh, mw);
    CP360_CHECK_HIP();
    return CP360_OK;
}
