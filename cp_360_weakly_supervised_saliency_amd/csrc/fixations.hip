// K15: fixation ground truth from scan-paths, and shuffled AUC on the sphere.  A video's fixations are N points (longitude,
// latitude in radians, float64) in CSR form: offsets int32 [F + 1], the points of frame f are offsets[f] .. offsets[f + 1] - 1.
// The specification is the package's own, DESIGN.md "K15"; tests/fixations_restate.py restates it in float64 and exact integers.
//
//   bin      u = (lon / pi + 1) (w / 2), x = floor(u) mod w in 0 .. w - 1;  v = (1 - lat / (pi / 2)) (h / 2), y = clamp(floor(v), 0,
//            h - 1): float64, one operation per step, no trigonometry - numpy gives the same integers.  A point with a non-finite
//            coordinate contributes nothing anywhere; a finite longitude so large that u overflows lands in column 0.
//   counts   counts[f, y, x] = the number of frame f's points in pixel (x, y), n_points[f] = the number of its finite points
//   density  G[f, i] = sum_k e(p_i, q_k) over the frame's finite points in ascending k, e = expf(kappa (p_i . q_k - 1)), kappa =
//            1 / sigma^2 rounded once (K12's convention), p_i from sphere.h's tables, q_k = dir(lon_k, lat_k) in double, rounded
//            to f32; the sum is f32 in that order: a frame's map does not depend on F or on its place in the batch
//   sAUC     K14's construction with multiplicities: positives pos_i (clamped to 0 .. 1023), negatives neg_i (0 .. 2^20, every
//            pixel, fixated ones included), C_tot = sum pos, A_neg = sum neg.  For a pixel with pos_i > 0: C_i = sum_{pos_j > 0,
//            S_j >= S_i} pos_j, A_i = sum_{S_j >= S_i} neg_j.  The ROC points are (0, 0), the distinct (A_i / A_neg, C_i / C_tot)
//            by descending S_i, (1, 1); N = sum_k (A_k - A_k-1)(C_k + C_k-1) is an integer and AUC = N / (2 A_neg C_tot), rounded
//            once.  C_tot = 0, A_neg = 0, a non-finite S or 2 A_neg C_tot >= 2^53: NaN.  Summed by parts, with the distinct
//            positive values v_1 > .. > v_m, mult_k = sum of pos_j over S_j = v_k and A_k = sum of neg_j over S_j >= v_k:
//                N = 2 A_neg C_tot - T,   T = sum_{k = 1 .. m} A_k (mult_k + mult_k+1),   mult_m+1 = 0
//            Every term needs the A of its own value alone, T is a sum of non-negative terms below 2^53 (it never wraps, any
//            order gives the same bits) and it is linear in A.
//
// Launches, all on the caller's stream, no host synchronisation, integer atomics only (any order gives the same bits):
//   K15a  counts: a clear, then one workgroup per frame, a vector atomicAdd per point
//   K15b  density: grid (ceil(P / 256), F), a pixel per thread; the frame's q_k staged in LDS 256 at a time, every lane reads the
//         same address (a broadcast), one expf per pair
//   K15c  sAUC prepare: one 1024-thread workgroup per frame - the sums, the finiteness of S, the positives compacted as (S, pos)
//   K15d  sAUC rank: grid (ceil(P / 256), F), sized for P positives in tiles of 256.  A thread owns one positive, value v: a loop
//         over the compacted list gives meq = the sum of pos_j at v, whether the thread is the first of its ties in the list, and
//         (nl, mlow) = the largest value below v and the sum of pos_j at it, tracked online in the one pass; a loop over pixels,
//         (S_j, neg_j) staged in LDS 1024 at a time, gives A with one compare-select-add per pair (u32 per tile: 1024 * 2^20 <
//         2^32; 64 bits across tiles).  The first of each distinct value adds A (meq + mlow) to the frame's T.  A video has tens
//         of positives per frame, not P: the workgroups that the positives leave over split the pixel loop (T is linear in A)
//         as far as kSplit allows, the rest exit at once.
//   K15e  sAUC finish: the quotient
//
// K19: the human ceiling and the prior baselines, one score pair per fixation point (DESIGN.md "K19"; tests/ceiling_restate.py).
// Point k of frame f lies in pixel i_k (the binning above) and is scored against a map l_k f64 [P]:
//   leave-one-out  l_k[j] = max(T_f[j] - (double)e_k(j), 0): T_f[j] = sum_k (double)e_k(j) over the frame's finite points in
//                  ascending k, e_k(j) K15b's f32 term.  The subtraction stands for the sum over the other viewers: a video
//                  costs N P terms, not N n P.
//   map            l_k[j] = (double)S[f or 0][j]
//   scores         mu = sum_a l_k / A, sigma = sqrt(sum_a (l_k - mu)^2 / A), nss = (l_k[i_k] - mu) / sigma;  A_k = sum of a_j over
//                  j != i_k with l_k[j] >= l_k[i_k], A_neg = A - a_{i_k}, auc = (double)(2 A_neg - A_k) / (2.0 (double)A_neg): K14's
//                  AUC-Judd with the one fixated pixel i_k.  NaN for both: a point with a non-finite coordinate, a point that no
//                  frame owns, a non-finite value in the frame's S.
//   K19a  totals: K15b's kernel with an f64 sum, T to the workspace
//   K19b  scores: a wave per point, four points per workgroup (K17b's shape); l_k[i_k] first (every lane the same), pass 1 strides
//         over the pixels for sum_a l and, in int32 per lane, A and A_k, pass 2 for the centred sum; each pass recomputes e_k(j)
//         from the tables: two expf per (point, pixel) pair.  wave_sum_down in its fixed order, no LDS, no barrier, no atomics: a
//         point's two numbers do not depend on F, N or the point's place in the batch.
#pragma clang fp contract(off)
#include "roc.h"

#include <math.h>

namespace {

constexpr int kFixTile = 256;                // K15b: points staged at a time
constexpr int kMaxPos = 1023;
constexpr int kMaxNeg = 1 << 20;
constexpr int kPointWaves = 4;               // K19b: points (waves) per workgroup
constexpr int kMaxWeight = 1024;             // K19b: the row weights, as K14 clamps them
// K15d: a workgroup that shares a tile's pixel loop repeats the tile's list loop (n entries), so it takes a share only while the
// share is at least kSplit n pixels.  Measured on one MI355X, cp360_fix_sauc alone at the bench shape (256 frames of 120 x 240,
// n = 25 .. 32, 29 pixel tiles; three runs each): kSplit 4 (113 chunks) 0.162 / 0.164 / 0.162 ms, 16 (60 chunks) 0.138 / 0.138 /
// 0.139 ms, 64 (15 chunks of two pixel tiles) 0.132 / 0.134 / 0.132 ms.
constexpr int kSplit = 64;
constexpr double kPi = 3.14159265358979323846;
constexpr double kHalfPi = 1.57079632679489661923;

struct SaucHdr {                             // per frame, K15c -> K15d, K15e
    int n_rank;                              // the number of positive pixels, or 0 when the frame has no AUC
    int pad;
    long long c_tot, a_neg;
    unsigned long long T;                    // sum_k A_k (mult_k + mult_k+1)
};

struct FixLayout {
    size_t hdr, cs, cp, total;                   // byte offsets, behind sphere.h's tables
};

// F = 0: the tables alone (counts needs nothing, density the tables)
FixLayout fix_layout(int F, int h, int w) {
    FixLayout l;
    const size_t n = (size_t)F * (size_t)h * (size_t)w;
    l.hdr = tab_bytes(h, w);
    l.cs = l.hdr + align16((size_t)F * sizeof(SaucHdr));
    l.cp = l.cs + align16(n * sizeof(float));
    l.total = l.cp + align16(n * sizeof(unsigned));
    return l;
}

__device__ __forceinline__ bool fix_finite(double v) { return fabs(v) < INFINITY; }

// the pixel of (lon, lat); false for a point that contributes nothing
__device__ __forceinline__ bool fix_bin(double lon, double lat, int h, int w, int& x, int& y) {
    if (!fix_finite(lon) || !fix_finite(lat)) return false;
    const double u = (lon / kPi + 1.0) * ((double)w / 2.0);
    const double v = (1.0 - lat / kHalfPi) * ((double)h / 2.0);
    double xf = fmod(floor(u), (double)w);                             // exact; NaN when u overflowed
    if (xf < 0.0) xf += (double)w;
    x = xf >= 0.0 && xf < (double)w ? (int)xf : 0;
    const double yf = floor(v);
    y = yf < 0.0 ? 0 : (yf > (double)(h - 1) ? h - 1 : (int)yf);
    return true;
}

// q = dir(lon, lat) in double, rounded to f32, and 1 for a finite point; zeros for one that is dropped
__device__ __forceinline__ float4 fix_dir(double lon, double lat) {
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (fix_finite(lon) && fix_finite(lat)) {
        const double cl = cos(lat);
        q = make_float4((float)(cl * cos(lon)), (float)sin(lat), (float)(cl * sin(lon)), 1.f);
    }
    return q;
}

// ------------------------------------------------------------------ K15a: counts
// grid F, 256 threads; counts cleared before
__global__ __launch_bounds__(256) void fix_counts_kernel(const double* __restrict__ lonlat, const int* __restrict__ offsets, int N,
                                                         int h, int w, int* __restrict__ counts, int* __restrict__ n_points) {
    __shared__ int red[4];
    const int f = blockIdx.x, tid = threadIdx.x;
    int k0, k1;
    fix_range(offsets, f, N, k0, k1);
    int* c = counts + (size_t)f * h * w;
    int n = 0;
    for (long long k = (long long)k0 + tid; k < k1; k += 256) {
        int x, y;
        if (fix_bin(lonlat[2 * k], lonlat[2 * k + 1], h, w, x, y)) {
            atomicAdd(&c[y * w + x], 1);
            ++n;
        }
    }
    n = wave_sum_down(n);
    if ((tid & 63) == 0) red[tid >> 6] = n;
    __syncthreads();
    if (tid == 0) n_points[f] = waves4_sum(red, 1);
}

// ------------------------------------------------------------------ K15b: density (T = float), K19a: totals (T = double)
// grid (ceil(P / 256), F), 256 threads; the terms are f32 for both, T is the type of the sum and of out
template <typename T>
__global__ __launch_bounds__(256) void fix_density_kernel(const double* __restrict__ lonlat, const int* __restrict__ offsets, int N,
                                                          const float2* __restrict__ tabx, const float2* __restrict__ taby,
                                                          T* __restrict__ out, int h, int w, float kappa) {
    __shared__ float4 tile_q[kFixTile];                                // q_k, and 1 for a finite point, 0 for one that is dropped
    const int P = h * w, tid = threadIdx.x, f = blockIdx.y;
    const int i = blockIdx.x * 256 + tid;
    int k0, k1;
    fix_range(offsets, f, N, k0, k1);
    float px = 1.f, py = 0.f, pz = 0.f;
    if (i < P) {
        const int y = i / w, x = i - y * w;
        stab_dir(tabx[x], taby[y], px, py, pz);
    }
    T acc = (T)0.f;
    for (long long t0 = k0; t0 < k1; t0 += kFixTile) {                 // k0, k1 are the workgroup's: the barriers are uniform
        const long long k = t0 + tid;
        if (k < k1) tile_q[tid] = fix_dir(lonlat[2 * k], lonlat[2 * k + 1]);
        __syncthreads();
        const int n = k1 - t0 < kFixTile ? (int)(k1 - t0) : kFixTile;
        for (int k = 0; k < n; ++k) {
            const float4 q = tile_q[k];
            const float e = vmf(kappa, px, py, pz, q.x, q.y, q.z);
            acc += (T)(q.w != 0.f ? e : 0.f);                          // acc >= +0: adding +0 changes no bit
        }
        __syncthreads();
    }
    if (i < P) out[(size_t)f * P + i] = acc;                           // a frame without points: zeros
}

// ------------------------------------------------------------------ K19b: the scores of every point
// the scored map of a point at pixel j, whose column and row entries of the tables are ctheta and cphi
template <bool kLoo>
__device__ __forceinline__ double point_map(const double* __restrict__ Tf, const float* __restrict__ Sf, int j, const float2 ctheta,
                                            const float2 cphi, float kappa, const float4 q) {
    if (!kLoo) return (double)Sf[j];
    float px, py, pz;
    stab_dir(ctheta, cphi, px, py, pz);
    const double e = (double)vmf(kappa, px, py, pz, q.x, q.y, q.z);    // K19a's term, bit for bit
    return fmax(Tf[j] - e, 0.0);
}

// grid ceil(N / 4), 256 threads; kLoo: T f64 [F, P] from K19a, else S f32 with s_stride = P or 0 floats between the frames
template <bool kLoo>
__global__ __launch_bounds__(64 * kPointWaves) void fix_point_scores_kernel(const float* __restrict__ S, size_t s_stride,
                                                                            const double* __restrict__ T, const double* __restrict__ lonlat,
                                                                            const int* __restrict__ offsets, int N, int F,
                                                                            const float2* __restrict__ tabx, const float2* __restrict__ taby,
                                                                            const int* __restrict__ weights, double* __restrict__ scores,
                                                                            int h, int w, float kappa) {
    const int lane = threadIdx.x & 63;
    const long long k = (long long)blockIdx.x * kPointWaves + (threadIdx.x >> 6);
    if (k >= N) return;                                                // the whole wave; the kernel has no barrier
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const int f = fix_frame(offsets, F, (int)k);
    int k0, k1, xi = 0, yi = 0;
    fix_range(offsets, f, N, k0, k1);
    const double lon = lonlat[2 * k], lat = lonlat[2 * k + 1];
    if (k < k0 || k >= k1 || !fix_bin(lon, lat, h, w, xi, yi)) {       // no frame owns the point, or it is dropped
        if (lane == 0) {
            scores[2 * k] = nan;
            scores[2 * k + 1] = nan;
        }
        return;
    }
    const int P = h * w, ik = yi * w + xi;
    const float4 q = fix_dir(lon, lat);
    const double* Tf = kLoo ? T + (size_t)f * P : nullptr;
    const float* Sf = kLoo ? nullptr : S + (size_t)f * s_stride;
    const double li = point_map<kLoo>(Tf, Sf, ik, tabx[xi], taby[yi], kappa, q);      // every lane the same
    const int ai = fix_clamp(weights[yi], 0, kMaxWeight);
    const int dx = 64 % w, dy = 64 / w;
    // pass 1: sum_a l, A, A_k and whether every value is finite; at most 2^15 pixels of weight 1024 a lane
    double s1 = 0.0;
    int at = 0, ak = 0, bad = 0;
    int x = lane % w, y = lane / w;
    for (int j = lane; j < P; j += 64) {
        const int a = fix_clamp(weights[y], 0, kMaxWeight);
        const double l = point_map<kLoo>(Tf, Sf, j, tabx[x], taby[y], kappa, q);
        s1 += (double)a * l;
        at += a;
        ak += j != ik && l >= li ? a : 0;
        bad += !(fabs(l) < INFINITY);
        x += dx;
        y += dy;
        if (x >= w) {
            x -= w;
            ++y;
        }
    }
    const double sum1 = __shfl(wave_sum_down(s1), 0, 64);
    const long long A = __shfl(wave_sum_down((long long)at), 0, 64);
    const long long Ak = wave_sum_down((long long)ak);
    const int nbad = wave_sum_down(bad);
    const double mu = sum1 / (double)A;
    // pass 2: the centred sum
    double s2 = 0.0;
    x = lane % w;
    y = lane / w;
    for (int j = lane; j < P; j += 64) {
        const double a = (double)fix_clamp(weights[y], 0, kMaxWeight);
        const double d = point_map<kLoo>(Tf, Sf, j, tabx[x], taby[y], kappa, q) - mu;
        s2 += a * (d * d);
        x += dx;
        y += dy;
        if (x >= w) {
            x -= w;
            ++y;
        }
    }
    s2 = wave_sum_down(s2);
    if (lane == 0) {
        const double sigma = sqrt(s2 / (double)A);
        const long long a_neg = A - ai;
        const bool ok = nbad == 0;
        scores[2 * k] = ok ? (double)(2 * a_neg - Ak) / (2.0 * (double)a_neg) : nan;   // A_neg = 0: 0 / 0
        scores[2 * k + 1] = ok ? (li - mu) / sigma : nan;
    }
}

// ------------------------------------------------------------------ K15c: sums and the compacted positives
// grid F, 1024 threads
__global__ __launch_bounds__(kRocThreads) void fix_sauc_prep_kernel(const float* __restrict__ S, const int* __restrict__ pos,
                                                                    const int* __restrict__ neg, size_t neg_stride, int P,
                                                                    double* __restrict__ auc, long long* __restrict__ c_tot_out,
                                                                    long long* __restrict__ a_neg_out, SaucHdr* __restrict__ hdr,
                                                                    float* __restrict__ cs, unsigned* __restrict__ cp) {
    __shared__ long long sml[kRocWaves * 3];
    __shared__ int cnt;
    const int tid = threadIdx.x, f = blockIdx.x;
    S += (size_t)f * P;
    pos += (size_t)f * P;
    neg += (size_t)f * neg_stride;
    cs += (size_t)f * P;
    cp += (size_t)f * P;
    if (tid == 0) cnt = 0;
    __syncthreads();
    long long acc[3] = {0, 0, 0};                                      // C_tot, A_neg, non-finite values
    for (int i0 = 0; i0 < P; i0 += kRocThreads) {                      // uniform: ballots need every lane
        const int i = i0 + tid;
        int m = 0;
        float s = 0.f;
        if (i < P) {
            s = S[i];
            m = fix_clamp(pos[i], 0, kMaxPos);
            acc[0] += m;
            acc[1] += fix_clamp(neg[i], 0, kMaxNeg);
            acc[2] += !(fabsf(s) < INFINITY);
        }
        const bool fx = m > 0;
        const int slot = roc_slot(fx, &cnt);
        if (fx) {
            cs[slot] = s;
            cp[slot] = (unsigned)m;
        }
    }
    roc_reduce(acc, sml, RocAdd());
    if (tid == 0) {
        const long long c_tot = acc[0], a_neg = acc[1], bad = acc[2];
        // 2 A_neg C_tot < 2^53  <=>  A_neg <= floor((2^52 - 1) / C_tot): the product itself may not fit 64 bits
        const bool rank = bad == 0 && c_tot > 0 && a_neg > 0 && a_neg <= ((1LL << 52) - 1) / c_tot;
        c_tot_out[f] = c_tot;
        a_neg_out[f] = a_neg;
        if (!rank) auc[f] = __longlong_as_double(0x7ff8000000000000LL);
        hdr[f].n_rank = rank ? cnt : 0;
        hdr[f].pad = 0;
        hdr[f].c_tot = c_tot;
        hdr[f].a_neg = a_neg;
        hdr[f].T = 0ull;
    }
}

// ------------------------------------------------------------------ K15d: T of every frame
// grid (ceil(P / 256), F), 256 threads
__global__ __launch_bounds__(kRankThreads) void fix_sauc_rank_kernel(const float* __restrict__ S, const int* __restrict__ neg,
                                                                     size_t neg_stride, SaucHdr* __restrict__ hdr,
                                                                     const float* __restrict__ cs, const unsigned* __restrict__ cp,
                                                                     int P) {
    __shared__ __attribute__((aligned(16))) float sv[kRankTile];
    __shared__ __attribute__((aligned(16))) unsigned sp[kRankTile];
    const int f = blockIdx.y, tid = threadIdx.x;
    const int n = hdr[f].n_rank;
    if (n == 0) return;                                                // the whole workgroup: before any barrier
    // the grid holds ceil(P / 256) >= tiles workgroups: workgroup b owns tile b % tiles of the positives and every chunks-th
    // pixel tile from b / tiles on; T is linear in A, so the parts add up
    const int tiles = (n + kRankThreads - 1) / kRankThreads, share = P / (kSplit * n);                 // kSplit n <= 2^27
    const int spare = (int)gridDim.x / tiles, chunks = share < 1 ? 1 : (share < spare ? share : spare);
    if ((int)blockIdx.x >= tiles * chunks) return;
    const int chunk = (int)blockIdx.x / tiles;
    const int k = ((int)blockIdx.x - chunk * tiles) * kRankThreads + tid;
    S += (size_t)f * P;
    neg += (size_t)f * neg_stride;
    cs += (size_t)f * P;
    cp += (size_t)f * P;
    const bool own = k < n;
    const bool busy = k - (tid & 63) < n;                              // the wave owns a positive: the others only stage and wait
    const float v = own ? cs[k] : INFINITY;
    // the positives alone: the multiplicity at v, the first of the ties, the next lower value and the multiplicity at it
    unsigned meq = 0u, mlow = 0u;
    float nl = -INFINITY;
    bool first = true;
    for (int t0 = 0; t0 < n; t0 += kRankTile) {
#pragma unroll
        for (int q = 0; q < kRankTile / kRankThreads; ++q) {
            const int jj = q * kRankThreads + tid, j = t0 + jj;
            sv[jj] = j < n ? cs[j] : -INFINITY;                        // padding: below every value, multiplicity 0
            sp[jj] = j < n ? cp[j] : 0u;
        }
        __syncthreads();
        const int lim = n - t0 < kRankTile ? n - t0 : kRankTile;
        for (int jj = 0; busy && jj < lim; ++jj) {
            const float s = sv[jj];
            const unsigned m = sp[jj];
            const bool eq = s == v;
            meq += eq ? m : 0u;
            first = first && !(eq && t0 + jj < k);
            const float c = s < v ? s : -INFINITY;
            mlow = c > nl ? m : mlow + (c == nl ? m : 0u);             // while nl = -inf this gathers every m: the first c > nl drops it
            nl = fmaxf(nl, c);
        }
        __syncthreads();
    }
    if (nl == -INFINITY) mlow = 0u;                                    // the lowest value: nothing below it
    // this chunk's pixels: their share of A
    unsigned long long A = 0ull;
    for (int t0 = chunk * kRankTile; t0 < P; t0 += chunks * kRankTile) {          // chunks <= 2^13: t0 stays below 2^24
#pragma unroll
        for (int q = 0; q < kRankTile / kRankThreads; ++q) {
            const int jj = q * kRankThreads + tid, j = t0 + jj;
            const bool in = j < P;
            sv[jj] = in ? S[j] : 0.f;
            sp[jj] = in ? (unsigned)fix_clamp(neg[j], 0, kMaxNeg) : 0u;     // a pixel past the frame counts nothing
        }
        __syncthreads();
        unsigned a = 0u;
#pragma unroll 4
        for (int jj = 0; busy && jj < kRankTile; jj += 4) {
            const float4 s = *reinterpret_cast<const float4*>(&sv[jj]);
            const uint4 p = *reinterpret_cast<const uint4*>(&sp[jj]);
            a += s.x >= v ? p.x : 0u;
            a += s.y >= v ? p.y : 0u;
            a += s.z >= v ? p.z : 0u;
            a += s.w >= v ? p.w : 0u;
        }
        A += a;
        __syncthreads();
    }
    unsigned long long part = own && first ? A * (unsigned long long)(meq + mlow) : 0ull;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off);
    if ((tid & 63) == 0 && part) atomicAdd(&hdr[f].T, part);           // integers: no order
}

// ------------------------------------------------------------------ K15e: the AUC
__global__ __launch_bounds__(256) void fix_sauc_finish_kernel(const SaucHdr* __restrict__ hdr, double* __restrict__ auc, int F) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F || hdr[f].n_rank == 0) return;                          // K15c wrote the NaN
    const unsigned long long a_neg = (unsigned long long)hdr[f].a_neg, c_tot = (unsigned long long)hdr[f].c_tot;
    const unsigned long long N = 2ull * a_neg * c_tot - hdr[f].T;      // integers below 2^53: one rounding
    auc[f] = (double)N / (2.0 * (double)a_neg * (double)c_tot);
}

// ------------------------------------------------------------------ host side
// the points: lonlat may be NULL when there are none
int fix_points(const double* lonlat, const int32_t* offsets, long long N, int F, int h, int w) {
    if (!offsets || (!lonlat && N > 0)) return CP360_ERR_NULL;
    const int st = roc_args(F, h, w);
    if (st != CP360_OK) return st;
    if (N < 0) return CP360_ERR_BAD_SHAPE;
    if (N >= (1LL << 31)) return CP360_ERR_UNSUPPORTED;
    if (((uintptr_t)lonlat & 7) != 0 || ((uintptr_t)offsets & 3) != 0) return CP360_ERR_ALIGN;
    return CP360_OK;
}

}  // namespace

// ------------------------------------------------------------------ C ABI
extern "C" size_t cp360_fix_work_bytes(int F, int h, int w) {
    if (roc_args(F == 0 ? 1 : F, h, w) != CP360_OK) return 0;          // F = 0: what density needs, the tables alone
    return fix_layout(F, h, w).total;
}

extern "C" int cp360_fix_counts(const double* lonlat, const int32_t* offsets, long long N, int F, int h, int w, int32_t* counts,
                                int32_t* n_points, void* stream) {
    if (!counts || !n_points) return CP360_ERR_NULL;
    const int st = fix_points(lonlat, offsets, N, F, h, w);
    if (st != CP360_OK) return st;
    if ((((uintptr_t)counts | (uintptr_t)n_points) & 3) != 0) return CP360_ERR_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, (size_t)F * h * w * sizeof(int32_t), s) != hipSuccess) return CP360_ERR_HIP;
    hipLaunchKernelGGL(fix_counts_kernel, dim3(F), dim3(256), 0, s, lonlat, (const int*)offsets, (int)N, h, w, (int*)counts,
                       (int*)n_points);
    CP360_CHECK_HIP();
    return CP360_OK;
}

extern "C" int cp360_fix_density(const double* lonlat, const int32_t* offsets, long long N, int F, int h, int w, double sigma_rad,
                                 float* out, void* work, size_t work_bytes, void* stream) {
    if (!out || !work) return CP360_ERR_NULL;
    int st = fix_points(lonlat, offsets, N, F, h, w);
    if (st != CP360_OK) return st;
    if (!(sigma_rad > 0.0) || !isfinite(sigma_rad)) return CP360_ERR_BAD_SHAPE;
    if (((uintptr_t)out & 3) != 0) return CP360_ERR_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    SphereTabs t;
    st = open_tabs(work, work_bytes, tab_bytes(h, w), h, w, s, &t);
    if (st != CP360_OK) return st;
    const float kappa = (float)(1.0 / (sigma_rad * sigma_rad));
    hipLaunchKernelGGL(fix_density_kernel<float>, dim3((h * w + 255) / 256, F), dim3(256), 0, s, lonlat, (const int*)offsets, (int)N, t.x,
                       t.y, out, h, w, kappa);
    CP360_CHECK_HIP();
    return CP360_OK;
}

extern "C" int cp360_fix_sauc(const float* S, const int32_t* pos, const int32_t* neg, int Fn, int F, int h, int w, double* auc,
                              long long* c_tot, long long* a_neg, void* work, size_t work_bytes, void* stream) {
    if (!S || !pos || !neg || !auc || !c_tot || !a_neg || !work) return CP360_ERR_NULL;
    const int st = roc_args(F, h, w);
    if (st != CP360_OK) return st;
    if (Fn != 1 && Fn != F) return CP360_ERR_BAD_SHAPE;
    if (!aligned16(work) || (((uintptr_t)auc | (uintptr_t)c_tot | (uintptr_t)a_neg) & 7) != 0 ||
        (((uintptr_t)S | (uintptr_t)pos | (uintptr_t)neg) & 3) != 0)
        return CP360_ERR_ALIGN;
    const int P = h * w;
    const FixLayout l = fix_layout(F, h, w);
    if (work_bytes < l.total) return CP360_ERR_BAD_SHAPE;
    char* wk = (char*)work;
    SaucHdr* hdr = (SaucHdr*)(wk + l.hdr);
    float* cs = (float*)(wk + l.cs);
    unsigned* cp = (unsigned*)(wk + l.cp);
    const size_t neg_stride = Fn == 1 ? 0 : (size_t)P;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(fix_sauc_prep_kernel, dim3(F), dim3(kRocThreads), 0, s, S, (const int*)pos, (const int*)neg, neg_stride, P,
                       auc, c_tot, a_neg, hdr, cs, cp);
    CP360_CHECK_HIP();
    hipLaunchKernelGGL(fix_sauc_rank_kernel, dim3((P + kRankThreads - 1) / kRankThreads, F), dim3(kRankThreads), 0, s, S,
                       (const int*)neg, neg_stride, hdr, (const float*)cs, (const unsigned*)cp, P);
    CP360_CHECK_HIP();
    hipLaunchKernelGGL(fix_sauc_finish_kernel, dim3((F + 255) / 256), dim3(256), 0, s, (const SaucHdr*)hdr, auc, F);
    CP360_CHECK_HIP();
    return CP360_OK;
}

extern "C" size_t cp360_fix_point_work_bytes(int F, int h, int w) {
    if (roc_args(F, h, w) != CP360_OK) return 0;
    return tab_bytes(h, w) + align16((size_t)F * (size_t)h * (size_t)w * sizeof(double));
}

extern "C" int cp360_fix_point_scores(const float* S, int Fs, const double* lonlat, const int32_t* offsets, long long N, int F, int h,
                                      int w, double sigma_rad, const int32_t* weights, double* scores, void* work, size_t work_bytes,
                                      void* stream) {
    if (!offsets || !weights || !work || ((!lonlat || !scores) && N > 0)) return CP360_ERR_NULL;
    if (bad_image(F, h, w) || N < 0) return CP360_ERR_BAD_SHAPE;
    if (S ? (Fs != 1 && Fs != F) : (!(sigma_rad > 0.0) || !isfinite(sigma_rad))) return CP360_ERR_BAD_SHAPE;
    if (roc_args(F, h, w) != CP360_OK || N >= (1LL << 31)) return CP360_ERR_UNSUPPORTED;
    if ((((uintptr_t)lonlat | (uintptr_t)scores) & 7) != 0 || (((uintptr_t)offsets | (uintptr_t)weights | (uintptr_t)S) & 3) != 0)
        return CP360_ERR_ALIGN;
    const size_t tabs = tab_bytes(h, w);
    int st = check_work(work, work_bytes, tabs + align16((size_t)F * (size_t)h * (size_t)w * sizeof(double)));
    if (st != CP360_OK || N == 0) return st;                           // no points: nothing to launch
    hipStream_t s = (hipStream_t)stream;
    SphereTabs t;
    st = launch_tables(work, h, w, s, &t);
    if (st != CP360_OK) return st;
    const int P = h * w;
    const dim3 grid((unsigned)((N + kPointWaves - 1) / kPointWaves)), block(64 * kPointWaves);
    if (S) {
        hipLaunchKernelGGL(fix_point_scores_kernel<false>, grid, block, 0, s, S, Fs == 1 ? (size_t)0 : (size_t)P, (const double*)nullptr,
                           lonlat, (const int*)offsets, (int)N, F, t.x, t.y, (const int*)weights, scores, h, w, 0.f);
        CP360_CHECK_HIP();
        return CP360_OK;
    }
    double* T = (double*)((char*)work + tabs);
    const float kappa = (float)(1.0 / (sigma_rad * sigma_rad));
    hipLaunchKernelGGL(fix_density_kernel<double>, dim3((P + 255) / 256, F), dim3(256), 0, s, lonlat, (const int*)offsets, (int)N, t.x,
                       t.y, T, h, w, kappa);
    CP360_CHECK_HIP();
    hipLaunchKernelGGL(fix_point_scores_kernel<true>, grid, block, 0, s, (const float*)nullptr, (size_t)0, (const double*)T, lonlat,
                       (const int*)offsets, (int)N, F, t.x, t.y, (const int*)weights, scores, h, w, kappa);
    CP360_CHECK_HIP();
    return CP360_OK;
}
