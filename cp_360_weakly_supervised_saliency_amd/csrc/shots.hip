// K13: shot detection - the signature of an equirectangular frame that a hard cut changes and a camera rotation does not: the
// colour histogram of the whole sphere, every pixel weighted by the solid angle of its row.  The reference has no counterpart; the
// specification is the package's own, DESIGN.md "K13", and tests/shots_restate.py restates it in integers.
//
//   a_y = floor(cos(phi_y) 1024 + 1/2), phi_y = (1 - (2 y + 1) / H) pi / 2 (sphere.h's rows); int32 [H], written by the host
//   sig[f, c, b] = sum of a_y over the pixels (y, x) of frame f with frames[f, y, x, c] >> 2 == b; int64 [F, 3, 64]
//   every sig[f, c, :] sums to T = W sum_y a_y
// Integers only: the result does not depend on the order of accumulation, on the launch geometry or on F.
//
// K13a reads every byte once.  A workgroup of 8 waves takes R consecutive rows of one frame, a wave one row at a time: the row's
// weight is a scalar, and the row is walked in 16-byte vectors from the 16-byte boundary at or below its first byte, 1 KiB per
// wave step, whatever the address of the frame (a vector that the row only partly covers - at most two per row - is masked byte
// by byte).  The histogram lives in LDS, 32 copies of 3 x 64 bins with the copy on the bank (dword c 2048 + b 32 + lane % 32), so
// that the 32 lanes an LDS instruction serves together never meet on a bank, whatever the image: a constant frame costs what a
// texture costs.  Each workgroup flushes u32 partial sums (R W 1024 < 2^32); K13b adds a frame's partials into int64.
#include "sphere.h"

namespace {

constexpr int kShotBins = 64, kShotCopies = 32, kShotChan = kShotBins * kShotCopies, kShotHist = 3 * kShotChan;
constexpr int kShotSig = 3 * kShotBins;
constexpr int kShotThreads = 512;            // K13a: 8 waves share one 24 KB histogram, 4 workgroups = 32 waves per CU
constexpr int kSumWaves = 16;                // K13b: waves per (frame, channel)
constexpr int kShotMaxW = 1 << 21;           // one row's u32 partial: W 1024 < 2^32 with room for R >= 1

// the 16 bytes of q: byte j belongs to the channel whose base is c[j % 3]
__device__ __forceinline__ void shot_add_word(unsigned* h, unsigned v, unsigned ca, unsigned cb, unsigned cc, unsigned cd, unsigned a) {
    atomicAdd(&h[ca + (((v >> 2) & 63u) << 5)], a);
    atomicAdd(&h[cb + (((v >> 10) & 63u) << 5)], a);
    atomicAdd(&h[cc + (((v >> 18) & 63u) << 5)], a);
    atomicAdd(&h[cd + ((v >> 26) << 5)], a);
}

__device__ __forceinline__ void shot_add_vec(unsigned* h, const uint4 q, unsigned c0, unsigned c1, unsigned c2, unsigned a) {
    shot_add_word(h, q.x, c0, c1, c2, c0, a);                          // bytes 0 .. 3
    shot_add_word(h, q.y, c1, c2, c0, c1, a);                          // 4 .. 7
    shot_add_word(h, q.z, c2, c0, c1, c2, a);                          // 8 .. 11
    shot_add_word(h, q.w, c0, c1, c2, c0, a);                          // 12 .. 15
}

// ------------------------------------------------------------------ K13a: the weighted histogram of R rows
// grid (ceil(H / R), F), 512 threads; part u32 [F, gridDim.x, 3, 64]
__global__ __launch_bounds__(kShotThreads) void shot_hist_kernel(const uint8_t* __restrict__ frames, const int* __restrict__ wrow,
                                                                 unsigned* __restrict__ part, int H, int W, int R) {
    __shared__ unsigned h[kShotHist];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int k = tid; k < kShotHist; k += kShotThreads) h[k] = 0u;
    __syncthreads();
    const int f = blockIdx.y;
    const int y0 = blockIdx.x * R;
    const int y1 = y0 + R < H ? y0 + R : H;
    const int rb = 3 * W;                                              // bytes of a row
    for (int y = y0 + wave; y < y1; y += kShotThreads / 64) {
        const unsigned a = (unsigned)wrow[y];
        const uint8_t* row = frames + ((size_t)f * H + y) * (size_t)rb;
        const int d = (int)((uintptr_t)row & 15);
        const uint8_t* base = row - d;                                 // 16-byte aligned; the row is [d, end) from here
        const int end = d + rb;
        // the channel of byte j of this lane's vector is (p + j) % 3 in the first step and moves on by one per step: a step is
        // 1024 = 1 (mod 3) bytes, a lane 16 = 1 (mod 3) bytes
        const unsigned p = (unsigned)(lane + 2 * d) % 3u, bank = (unsigned)(lane & 31);
        unsigned c0 = p * kShotChan + bank;
        unsigned c1 = (p == 2u ? 0u : p + 1u) * kShotChan + bank;
        unsigned c2 = (p == 0u ? 2u : p - 1u) * kShotChan + bank;
        // a vector that lies inside the row is loaded one step ahead of its use: its latency passes under the current step's adds
        int o = lane * 16;
        bool full = o >= d && o + 16 <= end;
        uint4 q = make_uint4(0u, 0u, 0u, 0u);
        if (full) q = *reinterpret_cast<const uint4*>(base + o);
        while (o < end) {
            const int on = o + 1024;
            const bool fulln = on + 16 <= end;                         // on >= 1024 > d
            uint4 qn = make_uint4(0u, 0u, 0u, 0u);
            if (fulln) qn = *reinterpret_cast<const uint4*>(base + on);
            if (full) {
                shot_add_vec(h, q, c0, c1, c2, a);
            } else {                                                   // the row's first or last vector: only the row's own bytes
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    if (o + j >= d && o + j < end) {
                        const unsigned c = j % 3 == 0 ? c0 : (j % 3 == 1 ? c1 : c2);
                        atomicAdd(&h[c + (((unsigned)base[o + j] >> 2) << 5)], a);
                    }
                }
            }
            const unsigned t = c0;
            c0 = c1;
            c1 = c2;
            c2 = t;
            o = on;
            q = qn;
            full = fulln;
        }
    }
    __syncthreads();
    if (tid < kShotSig) {                                              // bin tid of the 32 copies, each lane starting on its own bank
        unsigned s = 0u;
#pragma unroll
        for (int k = 0; k < kShotCopies; ++k) s += h[tid * kShotCopies + ((k + tid) & (kShotCopies - 1))];
        part[((size_t)f * gridDim.x + blockIdx.x) * kShotSig + tid] = s;
    }
}

// ------------------------------------------------------------------ K13b: a frame's partials into int64
// grid (3, F), 1024 threads: a lane owns a bin of one channel, wave w adds partials w, w + 16, .. (eight loads in flight), then
// the 16 waves' sums are added through LDS
__global__ __launch_bounds__(kSumWaves * 64) void shot_sum_kernel(const unsigned* __restrict__ part, long long* __restrict__ sig,
                                                                  int nblk) {
    __shared__ long long red[kSumWaves][kShotBins];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = blockIdx.x, f = blockIdx.y;
    const unsigned* p = part + (size_t)f * nblk * kShotSig + c * kShotBins + lane;
    long long s = 0;
#pragma unroll 8
    for (int k = wave; k < nblk; k += kSumWaves) s += (long long)p[(size_t)k * kShotSig];
    red[wave][lane] = s;
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int k = 1; k < kSumWaves; ++k) s += red[k][lane];
        sig[((size_t)f * 3 + c) * kShotBins + lane] = s;
    }
}

// ------------------------------------------------------------------ host side
// rows per workgroup: 16 (2 per wave) when that still gives the chip several workgroups per CU, else 8; fewer for very wide rows,
// so that a workgroup's u32 sums hold (R W 1024 <= 2^31)
int shot_rows(int F, int H, int W) {
    int R = (long long)F * ((H + 15) / 16) >= 1024 ? 16 : 8;
    while (R > 1 && (long long)R * W > kShotMaxW) R >>= 1;
    return R;
}

int shot_args(int F, int H, int W) {
    if (bad_image(F, H, W)) return CP360_ERR_BAD_SHAPE;
    if ((double)H * (double)W * 1024.0 >= 4611686018427387904.0) return CP360_ERR_UNSUPPORTED;     // T >= 2^62
    if (big_image(F, H, W) || W > kShotMaxW) return CP360_ERR_UNSUPPORTED;
    return CP360_OK;
}

// cos(pi t) for |t| <= 1/2, the argument reduced exactly
double shot_cospi(double t) {
    const double kPi = 3.14159265358979323846;
    t = fabs(t);
    return t > 0.25 ? sin(kPi * (0.5 - t)) : cos(kPi * t);
}

}  // namespace

// ------------------------------------------------------------------ C ABI
extern "C" int cp360_shot_weights_host(int H, int32_t* a, long long* total_per_width) {
    if (!a) return CP360_ERR_NULL;
    if (H < 1) return CP360_ERR_BAD_SHAPE;
    long long total = 0;
    for (int y = 0; y < H; ++y) {
        // phi_y / pi = (H - 2 y - 1) / (2 H): an exact numerator, so that rows y and H - 1 - y get the same weight
        const double t = ((double)H - 2.0 * (double)y - 1.0) / (2.0 * (double)H);
        a[y] = (int32_t)floor(shot_cospi(t) * 1024.0 + 0.5);
        total += a[y];
    }
    if (total_per_width) *total_per_width = total;
    return CP360_OK;
}

extern "C" size_t cp360_shot_work_bytes(int F, int H, int W) {
    if (shot_args(F, H, W) != CP360_OK) return 0;
    const int R = shot_rows(F, H, W);
    return align16((size_t)F * ((H + R - 1) / R) * kShotSig * sizeof(unsigned));
}

extern "C" int cp360_shot_signatures(const uint8_t* frames, int F, int H, int W, const int32_t* weights, long long* sig, void* work,
                                     size_t work_bytes, void* stream) {
    if (!frames || !weights || !sig || !work) return CP360_ERR_NULL;
    const int st = shot_args(F, H, W);
    if (st != CP360_OK) return st;
    if (!aligned16(work) || ((uintptr_t)sig & 7) != 0 || ((uintptr_t)weights & 3) != 0) return CP360_ERR_ALIGN;
    if (work_bytes < cp360_shot_work_bytes(F, H, W)) return CP360_ERR_BAD_SHAPE;
    const int R = shot_rows(F, H, W), nblk = (H + R - 1) / R;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(shot_hist_kernel, dim3(nblk, F), dim3(kShotThreads), 0, s, frames, (const int*)weights, (unsigned*)work, H, W,
                       R);
    CP360_CHECK_HIP();
    hipLaunchKernelGGL(shot_sum_kernel, dim3(3, F), dim3(kSumWaves * 64), 0, s, (const unsigned*)work, sig, nblk);
    CP360_CHECK_HIP();
    return CP360_OK;
}
