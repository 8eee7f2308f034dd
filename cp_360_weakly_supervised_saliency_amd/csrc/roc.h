// What the two files that compute a ROC on the sphere share: sphere_eval.hip (K14, AUC-Judd) and fixations.hip (K15, shuffled
// AUC).  Both take the exact integer ROC sum of a map against weighted positives and weighted negatives and divide once; K14 is
// K15 with pos_i = [i in M], neg_i = [i not in M] a_i, and the tests hold the two entries to the same bits (DESIGN.md "K14 and
// K15: one ROC").  Shared here: the launch shapes, the limits and their check, and the fixed-tree workgroup reduction and the
// wave compaction of the two prepare kernels.  The rank kernels stay apart, for a measured reason (same place).
// suploss.hip (K18, K14's KL, CC and NSS as a loss) takes the limits and the reduction from here too: its sums are K14a's.
// Everything here has internal linkage: each file that includes it compiles its own copy.
#pragma once
#include "sphere.h"

namespace {

constexpr int kRocThreads = 1024;            // the prepare kernels (K14a, K15c): one workgroup per frame
constexpr int kRocWaves = kRocThreads / 64;
constexpr int kRankThreads = 256;            // the rank kernels (K14b, K15d): positives per workgroup
constexpr int kRankTile = 1024;              // ... and pixels staged at a time = the span over which their u32 sums cannot overflow
constexpr int kRocMaxP = 1 << 21;            // 1023 P < 2^31 and 1024 P <= 2^31: C_tot, A and every partial sum fit a u32

int roc_args(int F, int h, int w) {
    if (bad_image(F, h, w)) return CP360_ERR_BAD_SHAPE;
    if (F > 65535 || (long long)h * w > kRocMaxP) return CP360_ERR_UNSUPPORTED;
    return CP360_OK;
}

// ---- workgroup reductions of the prepare kernels: 16 waves, each value through a xor butterfly (every lane ends with the same
// bits: a + b = b + a), then the 16 wave results through a second butterfly in every wave: one fixed tree
struct RocAdd { template <typename T> __device__ T operator()(T a, T b) const { return a + b; } };

template <typename T, int N, typename Op>
__device__ __forceinline__ void roc_reduce(T (&v)[N], T* sm, Op op) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int n = 0; n < N; ++n) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[n] = op(v[n], __shfl_xor(v[n], off));
        if (lane == 0) sm[wave * N + n] = v[n];
    }
    __syncthreads();
#pragma unroll
    for (int n = 0; n < N; ++n) {
        T r = sm[(lane & (kRocWaves - 1)) * N + n];                    // lane l holds wave l % 16's result
#pragma unroll
        for (int off = kRocWaves / 2; off > 0; off >>= 1) r = op(r, __shfl_xor(r, off));
        v[n] = r;
    }
    __syncthreads();
}

// ---- wave compaction of the prepare kernels: the slot of a kept lane in the workgroup's list, counted by the LDS counter *cnt.
// A wave's kept lanes take consecutive slots in lane order, the waves in the order their atomics land.  Every lane of the wave
// calls it (the ballot needs them all); the result means something for a kept lane alone.
__device__ __forceinline__ int roc_slot(bool keep, int* cnt) {
    const int lane = threadIdx.x & 63;
    const unsigned long long m = __ballot(keep);
    int base = 0;
    if (lane == 0 && m) base = atomicAdd(cnt, __popcll(m));
    base = __shfl(base, 0);
    return base + __popcll(m & ((1ull << lane) - 1ull));
}

}  // namespace
