// K14: saliency metrics on the sphere, a whole video per call - AUC-Judd, NSS, CC, SIM and KL of F saliency maps against F
// ground-truth maps on an h x w equirectangular grid, every pixel weighted by the solid angle of its row (K13's int32 table, a
// kernel argument: no trigonometry here).  The reference scores one flat frame per call (K8, metrics.hip, stays as it is); the
// specification of this file is the package's own, DESIGN.md "K14", and tests/sphere_eval_restate.py restates it in float64 and
// exact integers.
//
//   a_i = the weight of pixel i's row (clamped to 0 .. 1024), A = sum_i a_i, sum_a x = sum_i a_i x_i; everything below is f64
//   mu_S = sum_a S / A, sigma_S = sqrt(sum_a (S - mu_S)^2 / A), G alike
//   M    = the explicit fixation mask, or { i : G_i > mu_G + 2 sigma_G };  n_fix = |M|,  A_neg = sum_{i not in M} a_i
//   CC   = sum_a (S - mu_S)(G - mu_G) / sqrt(sum_a (S - mu_S)^2  sum_a (G - mu_G)^2)
//   SIM  = sum_i min(P_i, Q_i),  P_i = a_i (S_i - min S) / sum_a (S - min S),  Q_i alike from G
//   KL   = sum_i Q_i log(eps + Q_i / (P_i + eps)),  eps = 2^-52
//   NSS  = (1 / n_fix) sum_{i in M} (S_i - mu_S) / sigma_S
//   AUC  : for i in M, c_i = #{j in M : S_j >= S_i}, g_i = #{j in M : S_j > S_i}, A_i = sum_{j not in M, S_j >= S_i} a_j.  The ROC
//          points are (0, 0), (A_i / A_neg, c_i / n_fix) by descending S_i, (1, 1); tied fixations share a point.  Twice the
//          trapezoid sum times A_neg n_fix is the integer N = sum over the distinct points of (A_k - A_k-1)(c_k + c_k-1), the
//          point before k being the one with c = g_k; AUC = N / (2 A_neg n_fix): one rounding, whatever the order of summation.
//
// Three launches, no host synchronisation, no global float atomics:
//   K14a  one 1024-thread workgroup per frame: three passes over the frame (sums and minima; centred sums and masses; SIM, KL,
//         NSS, the mask), every thread adding its pixels tid, tid + 1024, .. in ascending order, the workgroup's sums added in a
//         fixed tree - the order depends on (h, w) alone, so a frame's numbers do not depend on F or on its place in the batch.
//         Leaves, for K14b: the fixated values compacted (in any order - ranks are counts, not positions), and per pixel the word
//         pk_j = 2^21 if j in M, else a_j.
//   K14b  grid (fixation tiles of 256, F): a thread owns one fixation, the workgroup stages 1024 pixels at a time in LDS as
//         (S_j, pk_j); every lane reads the same LDS address (a broadcast: no bank conflict), and one compare-select-add on the
//         packed word counts c and A at once: over 1024 pixels the weights sum to at most 2^20 < 2^21 and the count to at most
//         2^10, so the two fields of a u32 cannot meet.  g_i needs the fixated values alone: a second, short loop over the
//         compacted list (n_fix^2 compares, not n_fix P).  The point of fixation i goes to slot c_i - 1; tied fixations write the
//         same words to the same slot.  The grid is sized for n_fix = P; a tile past the frame's n_fix exits at once.
//   K14c  one workgroup per frame adds N over the filled slots (integers: no order) and writes the AUC.
//
// This AUC is fixations.hip's shuffled AUC (K15) with pos_i = [i in M], neg_i = [i not in M] a_i: the tests hold the two entries
// to the same bits, and the limits, their check and the workgroup reduction are shared (roc.h).  K14b and K14c stay beside K15d
// because unit positives and weights <= 1024 let c ride in the packed word for nothing and make the slot index a rank: K15d, which
// has neither, finds each value's neighbour in a list loop of about 17 instructions per entry where K14b spends 2, and on it this
// file's bench call took 1.81 ms instead of 1.29 ms (DESIGN.md "K14 and K15: one ROC").
#include "roc.h"

#include <math.h>

namespace {

constexpr int kEvalThreads = kRocThreads;    // K14a
constexpr int kEvalWaves = kRocWaves;
// kRankThreads (K14b: fixations per workgroup) and kRankTile (K14b: pixels staged at a time = the span over which the packed
// word cannot overflow) are roc.h's
constexpr int kFixShift = 21;                // pk = 1 << 21 for a fixated pixel; weights <= 1024, 1024 * 1024 < 2^21
constexpr unsigned kWeightMask = (1u << kFixShift) - 1u;
constexpr int kMaxWeight = 1024;             // 1024 P <= 2^31 (roc.h's kRocMaxP): A and every A_i fit a u32
constexpr double kEvalEps = 2.220446049250313e-16;             // 2^-52

struct EvalHdr {                             // per frame, K14a -> K14b, K14c
    int n_rank;                              // n_fix, or 0 when the frame has no AUC (n_fix = 0 or P, A_neg = 0, a non-finite value)
    int pad;
    long long a_neg;
};

struct EvalLayout {
    size_t hdr, pk, fixs, pts, gs, total;
};

EvalLayout eval_layout(int F, int P) {
    EvalLayout l;
    const size_t n = (size_t)F * (size_t)P;
    l.hdr = 0;
    l.pk = align16((size_t)F * sizeof(EvalHdr));
    l.fixs = l.pk + align16(n * sizeof(unsigned));
    l.pts = l.fixs + align16(n * sizeof(float));
    l.gs = l.pts + align16(n * sizeof(uint2));
    l.total = l.gs + align16(n * sizeof(unsigned));
    return l;
}

struct EvMin { __device__ float operator()(float a, float b) const { return fminf(a, b); } };

__device__ __forceinline__ int eval_weight(const int* __restrict__ wrow, int y) {
    const int a = wrow[y];
    return a < 0 ? 0 : (a > kMaxWeight ? kMaxWeight : a);
}

// ------------------------------------------------------------------ resampling
// grid (ceil(h w / 256), F): dst[f](x, y) = bilinear(src[f], sx, sy), columns wrap, rows clamp; a source of the grid's size is copied
__global__ __launch_bounds__(256) void seval_resample_kernel(const float* __restrict__ src, int hs, int ws, float* __restrict__ dst,
                                                             int h, int w) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= h * w) return;
    const int f = blockIdx.y;
    const float* img = src + (size_t)f * hs * ws;
    float* out = dst + (size_t)f * h * w;
    if (hs == h && ws == w) {
        out[i] = img[i];
        return;
    }
    const int y = i / w, x = i - y * w;
    const float sx = (float)((double)((long long)(2 * x + 1) * ws) / (double)(2 * w) - 0.5);
    const float sy = (float)((double)((long long)(2 * y + 1) * hs) / (double)(2 * h) - 0.5);
    sphere_sample<float, 1>(img, hs, ws, sx, sy, out + i);
}

// ------------------------------------------------------------------ K14a: moments, SIM, KL, NSS, the mask
// grid F, 1024 threads.  scores f64 [F, 5] = (auc, nss, cc, sim, kl): the AUC is K14c's
__global__ __launch_bounds__(kEvalThreads) void seval_moments_kernel(const float* __restrict__ S, const float* __restrict__ G,
                                                                     const uint8_t* __restrict__ fix, const int* __restrict__ wrow,
                                                                     int h, int w, double* __restrict__ scores,
                                                                     int* __restrict__ n_fix_out, EvalHdr* __restrict__ hdr,
                                                                     unsigned* __restrict__ pk, float* __restrict__ fixs,
                                                                     uint2* __restrict__ pts) {
    __shared__ double smd[kEvalWaves * 5];
    __shared__ long long sml[kEvalWaves * 3];
    __shared__ float smf[kEvalWaves * 2];
    __shared__ int cnt;
    const int tid = threadIdx.x, f = blockIdx.x, P = h * w;
    S += (size_t)f * P;
    G += (size_t)f * P;
    if (fix) fix += (size_t)f * P;
    pk += (size_t)f * P;
    fixs += (size_t)f * P;
    pts += (size_t)f * P;
    if (tid == 0) cnt = 0;
    // pass 1: weighted sums, minima, A, and whether every value is finite
    double s1[2] = {0.0, 0.0};
    float mn[2] = {INFINITY, INFINITY};
    long long ia[3] = {0, 0, 0};                                       // A, non-finite values, (pass 3) -
    for (int i = tid; i < P; i += kEvalThreads) {
        const int a = eval_weight(wrow, i / w);
        const float s = S[i], g = G[i];
        s1[0] += (double)a * (double)s;
        s1[1] += (double)a * (double)g;
        mn[0] = fminf(mn[0], s);
        mn[1] = fminf(mn[1], g);
        ia[0] += a;
        ia[1] += !(fabsf(s) < INFINITY) || !(fabsf(g) < INFINITY);
    }
    {
        double t[5] = {s1[0], s1[1], 0.0, 0.0, 0.0};
        roc_reduce(t, smd, RocAdd());
        s1[0] = t[0];
        s1[1] = t[1];
    }
    roc_reduce(mn, smf, EvMin());
    roc_reduce(ia, sml, RocAdd());
    const double A = (double)ia[0];
    const bool bad = ia[1] != 0;
    const double mu_s = s1[0] / A, mu_g = s1[1] / A;
    const double min_s = (double)mn[0], min_g = (double)mn[1];
    // pass 2: centred sums and the masses above the minima
    double s2[5] = {0.0, 0.0, 0.0, 0.0, 0.0};                          // Css, Cgg, Csg, Ms, Mg
    for (int i = tid; i < P; i += kEvalThreads) {
        const double a = (double)eval_weight(wrow, i / w);
        const double s = (double)S[i], g = (double)G[i];
        const double ds = s - mu_s, dg = g - mu_g;
        s2[0] += a * (ds * ds);
        s2[1] += a * (dg * dg);
        s2[2] += a * (ds * dg);
        s2[3] += a * (s - min_s);
        s2[4] += a * (g - min_g);
    }
    roc_reduce(s2, smd, RocAdd());
    const double sig_s = sqrt(s2[0] / A), sig_g = sqrt(s2[1] / A);
    const double thr = mu_g + 2.0 * sig_g;
    const double mass_s = s2[3], mass_g = s2[4];
    // pass 3: the mask, SIM, KL, NSS; the fixated values compacted wave by wave (the loop is uniform: ballots need every lane)
    double s3[5] = {0.0, 0.0, 0.0, 0.0, 0.0};                          // SIM, KL, NSS sum
    long long i3[3] = {0, 0, 0};                                       // n_fix, A_neg
    for (int i0 = 0; i0 < P; i0 += kEvalThreads) {
        const int i = i0 + tid;
        const bool in = i < P;
        bool fx = false;
        float sf = 0.f;
        if (in) {
            const int ai = eval_weight(wrow, i / w);
            const double a = (double)ai;
            sf = S[i];
            const double s = (double)sf, g = (double)G[i];
            fx = fix ? fix[i] != 0 : g > thr;
            const double p = a * (s - min_s) / mass_s, q = a * (g - min_g) / mass_g;
            s3[0] += fmin(p, q);
            s3[1] += q * log(kEvalEps + q / (p + kEvalEps));
            if (fx) s3[2] += (s - mu_s) / sig_s;
            i3[0] += fx;
            i3[1] += fx ? 0 : ai;
            pk[i] = fx ? (1u << kFixShift) : (unsigned)ai;
        }
        const int slot = roc_slot(fx, &cnt);
        if (fx) fixs[slot] = sf;
    }
    roc_reduce(s3, smd, RocAdd());
    roc_reduce(i3, sml, RocAdd());
    const int n_fix = (int)i3[0];
    const long long a_neg = i3[1];
    const bool rank = !bad && n_fix > 0 && n_fix < P && a_neg > 0;
    for (int k = tid; k < n_fix; k += kEvalThreads) pts[k] = make_uint2(0u, 0u);      // c = 0: an empty slot
    if (tid == 0) {
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        const bool mass = mass_s > 0.0 && mass_g > 0.0;                // zero mass: 0 / 0, which fmin would drop
        double* o = scores + (size_t)f * 5;
        o[0] = nan;
        o[1] = bad || n_fix == P ? nan : s3[2] / (double)n_fix;
        o[2] = bad ? nan : s2[2] / sqrt(s2[0] * s2[1]);
        o[3] = bad || !mass ? nan : s3[0];
        o[4] = bad || !mass ? nan : s3[1];
        n_fix_out[f] = n_fix;
        hdr[f].n_rank = rank ? n_fix : 0;
        hdr[f].pad = 0;
        hdr[f].a_neg = a_neg;
    }
}

// ------------------------------------------------------------------ K14b: the ROC point of every fixation
// grid (ceil(P / 256), F), 256 threads
__global__ __launch_bounds__(kRankThreads) void seval_rank_kernel(const float* __restrict__ S, const EvalHdr* __restrict__ hdr,
                                                                  const unsigned* __restrict__ pk, const float* __restrict__ fixs,
                                                                  uint2* __restrict__ pts, unsigned* __restrict__ gs, int P) {
    __shared__ __attribute__((aligned(16))) float sv[kRankTile];
    __shared__ __attribute__((aligned(16))) unsigned sp[kRankTile];
    const int f = blockIdx.y, tid = threadIdx.x;
    const int n = hdr[f].n_rank;
    const int k = blockIdx.x * kRankThreads + tid;
    if ((int)(blockIdx.x * kRankThreads) >= n) return;                 // the whole workgroup: before any barrier
    S += (size_t)f * P;
    pk += (size_t)f * P;
    const bool own = k < n;
    const float v = own ? fixs[(size_t)f * P + k] : INFINITY;
    unsigned c = 0u, g = 0u, A = 0u;
    for (int t0 = 0; t0 < P; t0 += kRankTile) {
#pragma unroll
        for (int q = 0; q < kRankTile / kRankThreads; ++q) {
            const int jj = q * kRankThreads + tid, j = t0 + jj;
            const bool in = j < P;
            sv[jj] = in ? S[j] : 0.f;
            sp[jj] = in ? pk[j] : 0u;                                  // a pixel past the frame counts nothing
        }
        __syncthreads();
        unsigned ge = 0u;
#pragma unroll 4
        for (int jj = 0; jj < kRankTile; jj += 4) {
            const float4 s = *reinterpret_cast<const float4*>(&sv[jj]);
            const uint4 p = *reinterpret_cast<const uint4*>(&sp[jj]);
            ge += s.x >= v ? p.x : 0u;
            ge += s.y >= v ? p.y : 0u;
            ge += s.z >= v ? p.z : 0u;
            ge += s.w >= v ? p.w : 0u;
        }
        c += ge >> kFixShift;
        A += ge & kWeightMask;
        __syncthreads();
    }
    // g needs the fixated values alone: the frame's compacted list, n of them, staged the same way
    fixs += (size_t)f * P;
    for (int t0 = 0; t0 < n; t0 += kRankTile) {
#pragma unroll
        for (int q = 0; q < kRankTile / kRankThreads; ++q) {
            const int jj = q * kRankThreads + tid, j = t0 + jj;
            sv[jj] = j < n ? fixs[j] : -INFINITY;                      // below every value: counts nothing
        }
        __syncthreads();
        const int lim = n - t0 < kRankTile ? (n - t0 + 3) & ~3 : kRankTile;
#pragma unroll 4
        for (int jj = 0; jj < lim; jj += 4) {
            const float4 s = *reinterpret_cast<const float4*>(&sv[jj]);
            g += s.x > v;
            g += s.y > v;
            g += s.z > v;
            g += s.w > v;
        }
        __syncthreads();
    }
    if (own && c >= 1u && c <= (unsigned)n && g < c) {                 // always true for finite values: the slot is inside the frame's
        pts[(size_t)f * P + (c - 1u)] = make_uint2(A, c);
        gs[(size_t)f * P + (c - 1u)] = g;
    }
}

// ------------------------------------------------------------------ K14c: N and the AUC
// grid F, 256 threads
__global__ __launch_bounds__(256) void seval_auc_kernel(const EvalHdr* __restrict__ hdr, const uint2* __restrict__ pts,
                                                        const unsigned* __restrict__ gs, double* __restrict__ scores, int P) {
    __shared__ long long red[256];
    const int f = blockIdx.x, tid = threadIdx.x;
    const int n = hdr[f].n_rank;
    if (n == 0) return;                                                // K14a wrote the NaN
    pts += (size_t)f * P;
    gs += (size_t)f * P;
    long long N = 0;
    for (int k = tid; k < n; k += 256) {
        const uint2 pt = pts[k];
        if (pt.y != (unsigned)(k + 1)) continue;                       // empty: a tied fixation's slot
        const unsigned g = gs[k];
        const unsigned prev = g >= 1u && g <= (unsigned)k ? pts[g - 1u].x : 0u;
        N += (long long)(pt.x - prev) * (long long)(pt.y + g);
    }
    red[tid] = N;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) {
        const long long a_neg = hdr[f].a_neg;
        N = red[0] + (a_neg - (long long)pts[n - 1].x) * (2LL * n);    // the last point to (1, 1)
        scores[(size_t)f * 5] = (double)N / (2.0 * (double)a_neg * (double)n);
    }
}

}  // namespace

// ------------------------------------------------------------------ C ABI
extern "C" size_t cp360_seval_work_bytes(int F, int h, int w) {
    if (roc_args(F, h, w) != CP360_OK) return 0;
    return eval_layout(F, h * w).total;
}

extern "C" int cp360_seval_resample(const float* src, int F, int hs, int ws, float* dst, int h, int w, void* stream) {
    if (!src || !dst) return CP360_ERR_NULL;
    if (bad_image(F, hs, ws) || bad_image(F, h, w)) return CP360_ERR_BAD_SHAPE;
    const int st = roc_args(F, h, w);
    if (st != CP360_OK) return st;
    if (big_image(F, hs, ws)) return CP360_ERR_UNSUPPORTED;
    if (((uintptr_t)src & 3) != 0 || ((uintptr_t)dst & 3) != 0) return CP360_ERR_ALIGN;
    hipLaunchKernelGGL(seval_resample_kernel, dim3((h * w + 255) / 256, F), dim3(256), 0, (hipStream_t)stream, src, hs, ws, dst, h, w);
    CP360_CHECK_HIP();
    return CP360_OK;
}

extern "C" int cp360_seval_scores(const float* S, const float* G, const uint8_t* fixations, const int32_t* weights, int F, int h, int w,
                                  double* scores, int32_t* n_fix, void* work, size_t work_bytes, void* stream) {
    if (!S || !G || !weights || !scores || !n_fix || !work) return CP360_ERR_NULL;
    const int st = roc_args(F, h, w);
    if (st != CP360_OK) return st;
    if (!aligned16(work) || ((uintptr_t)scores & 7) != 0 || (((uintptr_t)S | (uintptr_t)G | (uintptr_t)weights | (uintptr_t)n_fix) & 3) != 0)
        return CP360_ERR_ALIGN;
    const int P = h * w;
    const EvalLayout l = eval_layout(F, P);
    if (work_bytes < l.total) return CP360_ERR_BAD_SHAPE;
    char* wk = (char*)work;
    EvalHdr* hdr = (EvalHdr*)(wk + l.hdr);
    unsigned* pk = (unsigned*)(wk + l.pk);
    float* fixs = (float*)(wk + l.fixs);
    uint2* pts = (uint2*)(wk + l.pts);
    unsigned* gs = (unsigned*)(wk + l.gs);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(seval_moments_kernel, dim3(F), dim3(kEvalThreads), 0, s, S, G, fixations, (const int*)weights, h, w, scores,
                       (int*)n_fix, hdr, pk, fixs, pts);
    CP360_CHECK_HIP();
    hipLaunchKernelGGL(seval_rank_kernel, dim3((P + kRankThreads - 1) / kRankThreads, F), dim3(kRankThreads), 0, s, S,
                       (const EvalHdr*)hdr, (const unsigned*)pk, (const float*)fixs, pts, gs, P);
    CP360_CHECK_HIP();
    hipLaunchKernelGGL(seval_auc_kernel, dim3(F), dim3(256), 0, s, (const EvalHdr*)hdr, (const uint2*)pts, (const unsigned*)gs, scores,
                       P);
    CP360_CHECK_HIP();
    return CP360_OK;
}
