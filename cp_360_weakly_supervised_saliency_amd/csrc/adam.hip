// K5o: the optimizer step of ConvLSTM training - torch.optim.Adam (amsgrad False, maximize False) in one pass over p, g, m, v
// that also writes the compute-dtype operands the next iteration reads, so nothing repacks after a step.
//
//   adam_flat_kernel        biases and any other tensor: grid-stride, 16-byte accesses, a scalar tail for n % 4
//   adam_conv_kernel<T,..>  a filter f32 OIHW [c_out, c_in, 3, 3]: one workgroup per (co tile x ci tile x 9 taps) as
//                           dgrad_pack_kernel (clstm_train.hip); p, g, m, v are read as contiguous OIHW runs, updated in
//                           registers and stored back in place; the rounded new p is staged in LDS and, after one barrier,
//                           written into each pack that was given, in runs contiguous along that pack's innermost dimension:
//                             tap-major forward pack      [row][tap][c_pad]                         (pack_weights_kernel)
//                             channel-major forward pack  [row / 256][c / BKS][tap][row % 256][BKS] (pack_weights_kernel)
//                             dgrad pack                  [ci - ci0][tap * c_out + co]              (dgrad_pack_kernel)
//                           row = the packed row of channel co (row_chan, tile.h).  Padding rows and columns are never
//                           written: they are zero from the first pack.
// Tiles: 32 x 32 (f32) and 64 x 64 (bf16), so every run is 128 bytes (64 in the channel-major pack, whose innermost
// dimension is 64 bytes; there 32 consecutive rows make one 2 KiB piece).  bf16 lanes store two elements (4 bytes).
//
// f32 arithmetic, IEEE division and square root, no atomics: every element is owned by one thread, a step is bit-reproducible.
#include "conv_common.h"
#include "../../include/cp360.h"

namespace {

struct AdamK {
    float wd, omb1, beta2, omb2, bc2_sqrt, eps, step_size;      // omb = 1 - beta; step_size = lr / bias_corr1
};

// torch/optim/adam.py, _single_tensor_adam: grad.add(param, alpha=wd); exp_avg.lerp_(grad, 1 - beta1);
// exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2); denom = sqrt(exp_avg_sq) / sqrt(bias_corr2) + eps;
// param.addcdiv_(exp_avg, denom, value=-lr / bias_corr1)
// Each line is one fused multiply-add where torch has a multiply and an add: one rounding fewer, never one more.
__device__ __forceinline__ void adam_update(float& p, float g, float& m, float& v, const AdamK& a) {
    if (a.wd != 0.f) g = __fmaf_rn(a.wd, p, g);
    m = __fmaf_rn(a.omb1, g - m, m);
    v = __fmaf_rn(a.omb2 * g, g, a.beta2 * v);
    // sqrtf, not __fsqrt_rn: without OCML_BASIC_ROUNDED_OPERATIONS that one is the native 1-ulp v_sqrt_f32; sqrtf and the division
    // are the refined, correctly rounded sequences (no fast-math in this build)
    const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
    p = __fmaf_rn(-a.step_size, m / denom, p);
}

__device__ __forceinline__ void adam_update4(float4& p, const float4& g, float4& m, float4& v, const AdamK& a) {
    adam_update(p.x, g.x, m.x, v.x, a);
    adam_update(p.y, g.y, m.y, v.y, a);
    adam_update(p.z, g.z, m.z, v.z, a);
    adam_update(p.w, g.w, m.w, v.w, a);
}

__global__ __launch_bounds__(256) void adam_flat_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                        float* __restrict__ m, float* __restrict__ v, long long n, AdamK a) {
    const long long n4 = n >> 2;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        float4 p4 = reinterpret_cast<float4*>(p)[i], m4 = reinterpret_cast<float4*>(m)[i], v4 = reinterpret_cast<float4*>(v)[i];
        const float4 g4 = reinterpret_cast<const float4*>(g)[i];
        adam_update4(p4, g4, m4, v4, a);
        reinterpret_cast<float4*>(p)[i] = p4;
        reinterpret_cast<float4*>(m)[i] = m4;
        reinterpret_cast<float4*>(v)[i] = v4;
    }
    const long long t = (n4 << 2) + threadIdx.x;                 // the n % 4 tail: threads 0 .. 2 of workgroup 0
    if (blockIdx.x == 0 && threadIdx.x < 3 && t < n) adam_update(p[t], g[t], m[t], v[t], a);
}

template <typename T> __device__ __forceinline__ T round_to(float v);
template <> __device__ __forceinline__ float round_to<float>(float v) { return v; }
template <> __device__ __forceinline__ bf16_raw round_to<bf16_raw>(float v) { return f32_to_bf16(v); }

// One lane's store: VEC consecutive elements of a pack (f32: one, bf16: two as one dword; the offsets are even).
template <typename T> struct Lane;
template <> struct Lane<float> {
    static constexpr int VEC = 1;
    static __device__ __forceinline__ void store(float* dst, const float* s, int stride) { *dst = s[0]; }
};
template <> struct Lane<bf16_raw> {
    static constexpr int VEC = 2;
    static __device__ __forceinline__ void store(bf16_raw* dst, const bf16_raw* s, int stride) {
        *reinterpret_cast<unsigned*>(dst) = (unsigned)s[0] | ((unsigned)s[stride] << 16);
    }
};

struct AdamPacks {
    void* tap;              // tap-major forward pack (NULL: none)
    void* chan;             // channel-major forward pack
    void* dgrad;            // dgrad pack of input channels [ci0, ci0 + n_dgrad)
    int c_pad_tap, c_pad_chan, ci0, n_dgrad;
};

template <typename T, int TCO, int TCI>
__global__ __launch_bounds__(256) void adam_conv_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                        float* __restrict__ m, float* __restrict__ v, int c_out, int c_in,
                                                        AdamK a, AdamPacks k) {
    constexpr int ROW = TCI * 9;                              // one output channel's OIHW run inside the tile
    constexpr int LDR = ROW + (sizeof(T) == 4 ? 1 : 2);       // row stride of 289 dwords: odd, as dgrad_pack_kernel's
    constexpr int RQ = ROW / 4;
    constexpr int VEC = Lane<T>::VEC;
    constexpr int BKS = 64 / (int)sizeof(T);                  // elements per 64-byte sub-step (pack_weights_kernel)
    __shared__ __attribute__((aligned(16))) T t[TCO * LDR];
    const int co0 = blockIdx.y * TCO, cb0 = blockIdx.x * TCI;
    const int ncol = min(TCI, c_in - cb0) * 9;                // c_in % 4 == 0: a multiple of 4
    const bool packs = k.tap || k.chan || k.dgrad;

    // two 16-byte pieces per thread and pass: eight loads in flight before the first store
    for (int base = threadIdx.x; base < TCO * RQ; base += 512) {
        float4 p4[2], g4[2], m4[2], v4[2];
        size_t e[2];
        int lds[2];
        bool ok[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int idx = base + 256 * u;
            const int r = idx / RQ, c = 4 * (idx - r * RQ);
            ok[u] = idx < TCO * RQ && co0 + r < c_out && c < ncol;
            lds[u] = r * LDR + c;
            e[u] = ((size_t)(co0 + r) * c_in + cb0) * 9 + c;
            if (ok[u]) {
                p4[u] = *reinterpret_cast<const float4*>(p + e[u]);
                g4[u] = *reinterpret_cast<const float4*>(g + e[u]);
                m4[u] = *reinterpret_cast<const float4*>(m + e[u]);
                v4[u] = *reinterpret_cast<const float4*>(v + e[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (!ok[u]) continue;
            adam_update4(p4[u], g4[u], m4[u], v4[u], a);
            *reinterpret_cast<float4*>(p + e[u]) = p4[u];
            *reinterpret_cast<float4*>(m + e[u]) = m4[u];
            *reinterpret_cast<float4*>(v + e[u]) = v4[u];
            if (packs) {
                T* s = t + lds[u];
                s[0] = round_to<T>(p4[u].x); s[1] = round_to<T>(p4[u].y); s[2] = round_to<T>(p4[u].z);
                s[3] = round_to<T>(p4[u].w);
            }
        }
    }
    if (!packs) return;
    __syncthreads();

    if (k.tap) {            // [row][tap][c_pad]: lanes along c
        T* out = reinterpret_cast<T*>(k.tap);
        constexpr int CV = TCI / VEC;
        for (int idx = threadIdx.x; idx < TCO * 9 * CV; idx += 256) {
            const int c = (idx % CV) * VEC, rt = idx / CV;
            const int tap = rt % 9, row = co0 + rt / 9;
            const int co = row_chan(row);
            if (co < c_out && cb0 + c < c_in)
                Lane<T>::store(out + ((size_t)row * 9 + tap) * k.c_pad_tap + cb0 + c, t + (co - co0) * LDR + c * 9 + tap, 9);
        }
    }
    if (k.chan) {           // [row / 256][c / BKS][tap][row % 256][BKS]: lanes along BKS, then along the rows
        T* out = reinterpret_cast<T*>(k.chan);
        constexpr int EV = BKS / VEC;
        const int cpb = k.c_pad_chan / BKS;
        for (int idx = threadIdx.x; idx < (TCI / BKS) * 9 * TCO * EV; idx += 256) {
            const int ev = (idx % EV) * VEC;
            int r = idx / EV;
            const int row = co0 + r % TCO;
            r /= TCO;
            const int tap = r % 9, cb = r / 9;
            const int c = cb * BKS + ev;
            const int co = row_chan(row);
            if (co < c_out && cb0 + c < c_in)
                Lane<T>::store(out + ((((size_t)(row >> 8) * cpb + (cb0 / BKS + cb)) * 9 + tap) * 256 + (row & 255)) * BKS + ev,
                               t + (co - co0) * LDR + c * 9 + tap, 9);
        }
    }
    if (k.dgrad) {          // [ci - ci0][tap * c_out + co]: lanes along co
        T* out = reinterpret_cast<T*>(k.dgrad);
        constexpr int OV = TCO / VEC;
        for (int idx = threadIdx.x; idx < TCI * 9 * OV; idx += 256) {
            const int col = (idx % OV) * VEC, rt = idx / OV;
            const int tap = rt % 9, cl = rt / 9;
            const int nl = cb0 + cl - k.ci0;
            if (nl >= 0 && nl < k.n_dgrad && co0 + col < c_out)
                Lane<T>::store(out + ((size_t)nl * 9 + tap) * c_out + co0 + col, t + col * LDR + cl * 9 + tap, LDR);
        }
    }
}

bool make_consts(double lr, double beta1, double beta2, double eps, double wd, double bc1, double bc2_sqrt, AdamK* a) {
    if (!(bc1 > 0.0) || !(bc2_sqrt > 0.0)) return false;
    *a = AdamK{(float)wd, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)bc2_sqrt, (float)eps,
               (float)(lr / bc1)};
    return true;
}

bool aligned16(const void* a, const void* b, const void* c, const void* d) {
    return ::aligned16(a) && ::aligned16(b) && ::aligned16(c) && ::aligned16(d);    // common.h's
}

}  // namespace

// ================================================================== C ABI (include/cp360.h, "K5o")
extern "C" int cp360_train_adam(float* p, const float* g, float* m, float* v, long long n, double lr, double beta1,
                                double beta2, double eps, double weight_decay, double bias_corr1, double bias_corr2_sqrt,
                                void* stream) {
    if (!p || !g || !m || !v) return CP360_ERR_NULL;
    AdamK a;
    if (n <= 0 || !make_consts(lr, beta1, beta2, eps, weight_decay, bias_corr1, bias_corr2_sqrt, &a)) return CP360_ERR_BAD_SHAPE;
    if (!aligned16(p, g, m, v)) return CP360_ERR_ALIGN;
    long long blocks = ((n >> 2) + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(adam_flat_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, a);
    CP360_CHECK_HIP();
    return CP360_OK;
}

extern "C" int cp360_train_adam_conv(float* p, const float* g, float* m, float* v, int c_out, int c_in, double lr,
                                     double beta1, double beta2, double eps, double weight_decay, double bias_corr1,
                                     double bias_corr2_sqrt, int dtype, void* fwd_tap_major, void* fwd_chan_major,
                                     void* dgrad_packed, int ci0, int n_dgrad, void* stream) {
    if (!p || !g || !m || !v) return CP360_ERR_NULL;
    AdamK a;
    if (c_out <= 0 || c_in <= 0 || !make_consts(lr, beta1, beta2, eps, weight_decay, bias_corr1, bias_corr2_sqrt, &a))
        return CP360_ERR_BAD_SHAPE;
    if (ci0 < 0 || n_dgrad < 0 || (long long)ci0 + n_dgrad > c_in || (dgrad_packed && n_dgrad == 0)) return CP360_ERR_BAD_SHAPE;
    if (dtype != CP360_F32 && dtype != CP360_BF16) return CP360_ERR_UNSUPPORTED;
    AdamPacks k{fwd_tap_major, fwd_chan_major, dgrad_packed, conv_c_pad(c_in, dtype, 0), conv_c_pad(c_in, dtype, 1), ci0, n_dgrad};
    if ((long long)c_out * c_in * 9 >= (1LL << 31) || (long long)conv_rows_pad(c_out) * 9 * k.c_pad_tap >= (1LL << 31))
        return CP360_ERR_UNSUPPORTED;
    const bool packs = fwd_tap_major || fwd_chan_major || dgrad_packed;
    if (c_in % 4 != 0 || (packs && c_out % 4 != 0) || !aligned16(p, g, m, v) ||
        (((uintptr_t)fwd_tap_major | (uintptr_t)fwd_chan_major | (uintptr_t)dgrad_packed) & 3))
        return CP360_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == CP360_F32)
        hipLaunchKernelGGL((adam_conv_kernel<float, 32, 32>), dim3((c_in + 31) / 32, (c_out + 31) / 32), dim3(256), 0, st, p, g,
                           m, v, c_out, c_in, a, k);
    else
        hipLaunchKernelGGL((adam_conv_kernel<bf16_raw, 64, 64>), dim3((c_in + 63) / 64, (c_out + 63) / 64), dim3(256), 0, st, p,
                           g, m, v, c_out, c_in, a, k);
    CP360_CHECK_HIP();
    return CP360_OK;
}
