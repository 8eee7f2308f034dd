// K3c: CubePad(1) + 3x3 convolution 64 -> 64 (+ folded BN, ReLU) on 56x56 cube faces - layer1's conv2 of
// model/resnet_cubic.py:85-106 at cube size 224 - as a resident-band MFMA kernel for 16-bit types.
//
// The generic implicit GEMM gathers a 128-byte im2col row per output pixel and TAP: nine times the
// activation tensor through the L2 -> LDS path, which bounds it (0.25 ms per conv, 330 TFLOP/s;
// DESIGN.md).  Here a workgroup owns a band of 4 output rows of one face:
//   * the 6 x 58 cube-padded pixels the band needs (348 x 128 B = 44.5 KB) are gathered ONCE by
//     LDS-DMA, each lane fetching through cubepad_src() (the halo comes from the neighbouring faces);
//   * the MFMA B fragment of (output pixel x, tap (ky, kx), k-chunk) is 16 bytes of patch pixel
//     (row + ky) * 58 + x + kx: the nine taps read the same resident pixels, no im2col copy;
//   * the 8 KiB weight slice of a tap streams through a three-slot LDS ring (L2-resident, 74 KB total).
// Patch swizzle: chunk c of pixel p sits at chunk c ^ (2 * ((p >> 1) & 3)); with 128-byte pixels this
// keeps every 16-lane ds_read_b128 group (16 consecutive pixels starting ANYWHERE, two chunk values)
// on 16 distinct 16-byte bank slots (exhaustive search, as for the clip kernel).
// Wave w computes output row w of the band: 56 pixels as 4 MFMA pixel blocks (8 of the 64 columns are
// padding) x 64 channels.  Two workgroups (256 threads, 68 KiB LDS) share a CU, so one band's gather /
// epilogue overlaps the other's MFMAs.  Epilogue: bias + ReLU, one rounding, 16-byte pieces (acc_chan).
// The tile primitives used here (vector types, mma_chunk, glds16, swizzles, acc_chan / row_chan, pack8 / unpack8, g_zero16): tile.h;
// the band gather, the epilogue piece and the host-side dispatch / checks shared with the other fused kernels: band.h.
#include "band.h"

namespace {
constexpr int N = 56, NP = N + 2, C = 64, BAND = 4;
constexpr int PATCH_PX = (BAND + 2) * NP;                    // 348
constexpr int PATCH_INST = (PATCH_PX + 7) / 8;               // 44 DMA instructions of 8 pixels x 128 B
constexpr int PATCH_LDS = PATCH_INST * 1024;                 // 45,056
constexpr int W_TAP = 64 * 128;                              // 8 KiB: one tap's 64 rows x 64 channels
constexpr int W_SLOTS = 3;
}  // namespace

// packed weights: [tap][row r][64 channels], row r <- output channel in acc_chan order, BN scale folded
template <typename T>
__global__ __launch_bounds__(256) void band3x3_pack_kernel(const float* __restrict__ w, const float* __restrict__ scale,
                                                           T* __restrict__ packed) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= 9 * 64 * 64) return;
    const int c = idx & 63, r = (idx >> 6) & 63, tap = idx >> 12;
    const int n = (r & ~31) + ((r >> 2) & 3) * 8 + ((r >> 4) & 1) * 4 + (r & 3);      // = row_chan(r)
    const float v = w[(n * 64 + c) * 9 + tap] * (scale ? scale[n] : 1.f);
    store_folded(packed, idx, v);
}

template <typename T>
__global__ __launch_bounds__(256, 2) void band3x3_kernel(const T* __restrict__ x, const T* __restrict__ wpk,
                                                         const float* __restrict__ bias, T* __restrict__ out, int relu) {
    __shared__ __attribute__((aligned(1024))) unsigned char lds[PATCH_LDS + W_SLOTS * W_TAP];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned lds_base = (unsigned)(size_t)lds;
    const int tile = blockIdx.x, img = tile / (N / BAND), band = tile - img * (N / BAND);
    const int grp = img / 6, f = img - grp * 6;
    const CubePadGeom geom{N, 1, 1, 1, 1};

    // ---- gather the band's padded pixels: instruction i = patch pixels 8i .. 8i+7, 128 B each
    CP360_GATHER_BAND_PATCH(x + (size_t)grp * 6 * N * N * C, C, f, BAND * band, NP, geom, PATCH_PX, PATCH_INST, 8, px_swz(q_), lds_base, wave, lane)
    // weight slice of tap t -> ring slot s: 8 instructions of 8 rows x 128 B, two per wave
    const unsigned char* wb = reinterpret_cast<const unsigned char*>(wpk);
    auto load_w = [&](int t, int s) __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int inst = wave * 2 + q;
            const int row = inst * 8 + (lane >> 3);
            const int chunk = (lane & 7) ^ ((row >> 1) & 7);
            glds16(wb + (size_t)t * W_TAP + row * 128 + chunk * 16,
                   __builtin_amdgcn_readfirstlane(lds_base + PATCH_LDS + s * W_TAP + inst * 1024));
        }
    };
    load_w(0, 0);
    load_w(1, 1);

    const int lrow = lane & 15, lchunk = lane >> 4;
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap) {
        // weights of `tap` landed (the patch DMAs are older); the next tap's two DMAs may still fly
        if (tap < 8) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        else         asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                                   // ... for every wave; slot (tap+2)%3 is free
        if (tap + 2 < 9) load_w(tap + 2, (tap + 2) % W_SLOTS);
        const int ky = tap / 3, kx = tap - ky * 3;
        const unsigned char* Ws = lds + PATCH_LDS + (tap % W_SLOTS) * W_TAP;
        const int pbase = (wave + ky) * NP + kx + lrow;    // patch pixel of this lane in pixel block 0
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            u32x4 a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = *reinterpret_cast<const u32x4*>(Ws + lds_swz(i * 16 + lrow, kk * 4 + lchunk));
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int p = pbase + 16 * j;
                b[j] = *reinterpret_cast<const u32x4*>(lds + p * 128 + (((kk * 4 + lchunk) ^ px_swz(p)) << 4));
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) mma_chunk<T>(acc[i][j], a[i], b[j]);
        }
    }
    // ---- epilogue: output row band*4 + wave of image img
    T* orow = out + ((size_t)img * N + band * BAND + wave) * N * C;
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) {
        const int n = pr * 32 + (lane >> 4) * 8;
        float bb[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) bb[e] = bias ? bias[n + e] : 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int xo = j * 16 + lrow;
            float v[8];
            CP360_BIAS_ACT8(v, acc[2 * pr][j], acc[2 * pr + 1][j], bb[e_], bb[4 + e_], CP360_NOACT)
            if (relu) {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = fmaxf(v[e], 0.f);
            }
            if (xo < N) *reinterpret_cast<u32x4*>(orow + (size_t)xo * C + n) = pack8(v, T());
        }
    }
}

extern "C" size_t cp360_band3x3_packed_bytes(int dtype) {
    return (dtype == CP360_BF16 || dtype == CP360_F16) ? (size_t)9 * W_TAP : 0;
}

extern "C" int cp360_band3x3_pack_weights(int dtype, const float* w_oihw, const float* scale, void* packed, void* stream) {
    if (!w_oihw || !packed) return CP360_ERR_NULL;
    return with_elem16(dtype, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL((band3x3_pack_kernel<T>), dim3(144), dim3(256), 0, (hipStream_t)stream, w_oihw, scale, (T*)packed);
    });
}

extern "C" int cp360_band3x3_forward(int dtype, const void* x, const void* packed, const float* bias, void* out,
                                     int n_img, int face, int channels, int relu, void* stream) {
    if (!x || !packed || !out) return CP360_ERR_NULL;
    if (const int bad = check_faces(n_img, face == N && channels == C, N, C)) return bad;      // other shapes: the generic implicit GEMM
    return with_elem16(dtype, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL((band3x3_kernel<T>), dim3((unsigned)(n_img * (N / BAND))), dim3(256), 0, (hipStream_t)stream, (const T*)x,
                           (const T*)packed, bias, (T*)out, relu);
    });
}
