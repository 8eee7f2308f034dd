// K5t: ConvLSTM training (temporal_model/train_temporal.py:87-170 of the reference, backward of model/clstm.py:54-80 and of
// the channel max of to_equi_nn, utils/cube_to_equi.py:37-66).  f32 and bf16 operands, f32 accumulation everywhere.
//
// Every gradient here is written by exactly one thread in a fixed order: no atomics, no split-K, so two identical
// iterations give bit-identical gradients.  The two scatters of the backward pass (CubePad's copies, the bilinear taps of
// the cube -> equirectangular sampling) are gathers over inverse tables built on the host.
//
//   train_gates_kernel          the forward gate epilogue of cp360_lstm_gates + the four activated gates kept for backward
//   train_gates_bwd_kernel      d(hidden), d(cell) -> d(gate pre-activations) (compute dtype: the next GEMM's operand), d(c_prev)
//   train_gemm_kernel<T, DGRAD> "full" correlation of dY with the 3x3 filter onto the zero-padded (face+2)^2 grid (f32)
//   cubepad_adjoint_kernel      sums the padded grid's copies back onto their CubePad source, ReLU mask of the saved activation
//   train_gemm_kernel<T, WGRAD> dW[co, ci, ky, kx] = sum over steps, faces, pixels of dY * CubePad(X), plus db = sum dY
//   sal_forward_kernel          to_equi_nn + channel max + the argmax channel (first maximum, as torch.max on the CPU)
//   sal_backward_kernel         d(map) -> d(hidden) through the argmax channel and the 4 bilinear taps
#include "conv_common.h"
#include "../../include/cp360.h"

#include <vector>

namespace {


template <typename T> __device__ __forceinline__ T from_f32(float v);
template <> __device__ __forceinline__ float from_f32<float>(float v) { return v; }
template <> __device__ __forceinline__ bf16_raw from_f32<bf16_raw>(float v) { return f32_to_bf16(v); }

// ------------------------------------------------------------------ gates, forward
template <typename T>
__global__ __launch_bounds__(256) void train_gates_kernel(const float* __restrict__ gp, int splits,
                                                          const float* __restrict__ bias, const float* __restrict__ c_prev,
                                                          float* __restrict__ c_next, T* __restrict__ h_out, int ld_h,
                                                          int h_coff, float* __restrict__ h_f32, float* __restrict__ acts,
                                                          int M, int Hc) {
    const long long total = (long long)M * Hc;
    const int G = 4 * Hc;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        const int m = (int)(idx / Hc), j = (int)(idx - (long long)m * Hc);
        float g[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = bias[k * Hc + j];
        for (int s = 0; s < splits; ++s) {
            const float* base = gp + ((size_t)s * M + m) * G + j;
#pragma unroll
            for (int k = 0; k < 4; ++k) g[k] += base[k * Hc];
        }
        const float ig = fast_sigmoid(g[0]), fg = fast_sigmoid(g[1]), og = fast_sigmoid(g[2]), cg = tanhf(g[3]);
        const float cn = fg * c_prev[(size_t)m * Hc + j] + ig * cg;
        const float hn = og * tanhf(cn);
        float* a = acts + (size_t)m * G + j;
        a[0] = ig; a[Hc] = fg; a[2 * Hc] = og; a[3 * Hc] = cg;
        c_next[(size_t)m * Hc + j] = cn;
        h_out[(size_t)m * ld_h + h_coff + j] = from_f32<T>(hn);
        if (h_f32) h_f32[(size_t)m * Hc + j] = hn;
    }
}

// ------------------------------------------------------------------ gates, backward
// c = f c_prev + i g, h = o tanh(c):  dc += dh o (1 - tanh^2 c);  d(pre-activation) = d(act) * act' from the saved outputs.
template <typename T>
__global__ __launch_bounds__(256) void train_gates_bwd_kernel(const float* __restrict__ dh, float* __restrict__ dc,
                                                              const float* __restrict__ acts, const float* __restrict__ c_prev,
                                                              const float* __restrict__ c_next, T* __restrict__ dgates, int M,
                                                              int Hc) {
    const long long total = (long long)M * Hc;
    const int G = 4 * Hc;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        const int m = (int)(idx / Hc), j = (int)(idx - (long long)m * Hc);
        const size_t e = (size_t)m * Hc + j;
        const float* a = acts + (size_t)m * G + j;
        const float ig = a[0], fg = a[Hc], og = a[2 * Hc], cg = a[3 * Hc];
        const float tc = tanhf(c_next[e]);
        const float gh = dh[e];
        const float gc = dc[e] + gh * og * (1.f - tc * tc);
        const float d_i = gc * cg, d_f = gc * c_prev[e], d_o = gh * tc, d_g = gc * ig;
        T* d = dgates + (size_t)m * G + j;
        d[0] = from_f32<T>(d_i * ig * (1.f - ig));
        d[Hc] = from_f32<T>(d_f * fg * (1.f - fg));
        d[2 * Hc] = from_f32<T>(d_o * og * (1.f - og));
        d[3 * Hc] = from_f32<T>(d_g * (1.f - cg * cg));
        dc[e] = gc * fg;                                  // d c_prev (read above, same element: in place)
    }
}

// ------------------------------------------------------------------ dgrad weight pack
// packed[n][tap * c_out + co] = W[co][ci0 + n][tap]: the B operand of the dgrad GEMM, K-contiguous.  32 x 32 (co, ci) tiles
// through LDS so that both the OIHW read and the packed write are contiguous.
template <typename T>
__global__ __launch_bounds__(256) void dgrad_pack_kernel(const float* __restrict__ w, T* __restrict__ packed, int c_out,
                                                         int c_in, int ci0, int n) {
    __shared__ float t[32][32 * 9 + 1];
    const int co0 = blockIdx.y * 32, nb = blockIdx.x * 32;
    const int K = 9 * c_out;
    for (int idx = threadIdx.x; idx < 32 * 288; idx += 256) {
        const int r = idx / 288, c = idx - r * 288;
        const int co = co0 + r, nl = nb + c / 9;
        t[r][c] = (co < c_out && nl < n) ? w[((size_t)co * c_in + ci0 + nl) * 9 + (c % 9)] : 0.f;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < 32 * 288; idx += 256) {
        const int nl = idx / 288, rest = idx - nl * 288;
        const int tap = rest / 32, col = rest - tap * 32;
        if (nb + nl < n && co0 + col < c_out)
            packed[(size_t)(nb + nl) * K + tap * c_out + co0 + col] = from_f32<T>(t[col][nl * 9 + tap]);
    }
}

// ------------------------------------------------------------------ the two GEMMs
// C[m, n] = sum_k A(m, k) B(k, n) on 64 x 64 tiles, 4 waves of 32 x 32, K steps of 32 staged through LDS (next step's
// operands prefetched into registers while the MFMAs of this one run).  f32: mfma_f32_16x16x4f32, bf16: mfma_f32_16x16x32_bf16.
//   DGRAD  A = dY at (py - ky, px - kx) of padded position m, k = tap * c_out + co (zero outside the face);  B = packed[n][k];
//          C -> f32 [M = n_img (face+2)^2, N]
//   WGRAD  A(m = co, k = pixel) = dY[k][co];  B(k, n = ci * 9 + tap) = X at CubePad(1) position (pixel + tap) (n = 9 c_in: 1);
//          C -> dW (OIHW f32: row m of C is dW[co] contiguous) and db
enum { DGRAD = 0, WGRAD = 1 };

struct GemmArgs {
    const void* a;          // dY
    const void* b;          // DGRAD: packed filter, WGRAD: X
    const int* tab;         // WGRAD: CubePad(1) source table [6, face+2, face+2]
    float* c;               // DGRAD: dXpad, WGRAD: dW
    float* db;              // WGRAD: bias gradient (NULL: none)
    int M, N, K;
    int face, c_out, c_in, ldx, accumulate;
};

template <typename T> struct Lds { static constexpr int LDK = 40; };
template <> struct Lds<float> { static constexpr int LDK = 33; };

template <typename T>
__device__ __forceinline__ void mma_step(f32x4 (&acc)[2][2], const T (*As)[Lds<T>::LDK], const T (*Bs)[Lds<T>::LDK],
                                         int wm, int wn, int lane);

template <>
__device__ __forceinline__ void mma_step<float>(f32x4 (&acc)[2][2], const float (*As)[33], const float (*Bs)[33], int wm,
                                                int wn, int lane) {
    const int r = lane & 15, q = lane >> 4;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        float a[2], b[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) a[i] = As[wm + i * 16 + r][4 * s + q];
#pragma unroll
        for (int j = 0; j < 2; ++j) b[j] = Bs[wn + j * 16 + r][4 * s + q];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
}

template <>
__device__ __forceinline__ void mma_step<bf16_raw>(f32x4 (&acc)[2][2], const bf16_raw (*As)[40], const bf16_raw (*Bs)[40],
                                                   int wm, int wn, int lane) {
    const int r = lane & 15, q = lane >> 4;
    u32x4 a[2], b[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) a[i] = *reinterpret_cast<const u32x4*>(&As[wm + i * 16 + r][8 * q]);
#pragma unroll
    for (int j = 0; j < 2; ++j) b[j] = *reinterpret_cast<const u32x4*>(&Bs[wn + j * 16 + r][8 * q]);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a[i]), __builtin_bit_cast(bf16x8, b[j]),
                                                                acc[i][j], 0, 0, 0);
}

template <typename T, int MODE>
__global__ __launch_bounds__(256) void train_gemm_kernel(GemmArgs g) {
    constexpr int LDK = Lds<T>::LDK;
    __shared__ __attribute__((aligned(16))) T As[64][LDK];
    __shared__ __attribute__((aligned(16))) T Bs[64][LDK];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
    const int wm = (wid >> 1) * 32, wn = (wid & 1) * 32;
    const T* A = reinterpret_cast<const T*>(g.a);
    const T* B = reinterpret_cast<const T*>(g.b);
    const int fp = g.face + 2, fsq = g.face * g.face;

    // DGRAD: element e of a thread = row (tid >> 5) + 8 e, column kk = tid & 31 of both tiles (K-contiguous loads)
    // WGRAD: element e = K row kk = 4 e + (tid >> 6), tile column tid & 63 (M / N-contiguous loads)
    int a_base[8];              // DGRAD: dY pixel (img, py, px) of row e, packed as img * fp^2 + py * fp + px (-1: row >= M)
    int b_n = 0, b_ci = 0, b_ky = 0, b_kx = 0;
    bool b_ones = false, b_ok = false;
    if (MODE == DGRAD) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int m = m0 + (tid >> 5) + 8 * e;
            a_base[e] = m < g.M ? m : -1;
        }
    } else {
        b_n = n0 + (tid & 63);
        b_ok = b_n < g.N;
        b_ones = b_n == 9 * g.c_in;
        b_ci = b_n / 9;
        const int tap = b_n - 9 * b_ci;
        b_ky = tap / 3;
        b_kx = tap - 3 * b_ky;
    }

    T ra[8], rb[8];
    auto load = [&](int k0) {
        if (MODE == DGRAD) {
            const int k = k0 + (tid & 31);
            const bool kok = k < g.K;
            const int tap = kok ? k / g.c_out : 0, co = k - tap * g.c_out;
            const int ky = tap / 3, kx = tap - 3 * ky;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                T v = from_f32<T>(0.f);
                const int m = a_base[e];
                if (kok && m >= 0) {
                    const int img = m / (fp * fp), r = m - img * fp * fp;
                    const int oy = r / fp - ky, ox = r % fp - kx;
                    if (oy >= 0 && oy < g.face && ox >= 0 && ox < g.face)
                        v = A[((size_t)(img * g.face + oy) * g.face + ox) * g.c_out + co];
                }
                ra[e] = v;
                const int n = n0 + (tid >> 5) + 8 * e;
                rb[e] = (kok && n < g.N) ? B[(size_t)n * g.K + k] : from_f32<T>(0.f);
            }
        } else {
            const int m = m0 + (tid & 63);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int k = k0 + 4 * e + (tid >> 6);
                const bool kok = k < g.K;
                ra[e] = (kok && m < g.M) ? A[(size_t)k * g.c_out + m] : from_f32<T>(0.f);
                T v = from_f32<T>(0.f);
                if (kok && b_ok) {
                    if (b_ones) {
                        v = from_f32<T>(1.f);
                    } else {
                        const int img = k / fsq, p = k - img * fsq;
                        const int oy = p / g.face, ox = p - oy * g.face, f = img % 6;
                        const int src = g.tab[(f * fp + oy + b_ky) * fp + ox + b_kx];
                        v = B[((size_t)(img - f) * fsq + src) * g.ldx + b_ci];
                    }
                }
                rb[e] = v;
            }
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (MODE == DGRAD) {
                As[(tid >> 5) + 8 * e][tid & 31] = ra[e];
                Bs[(tid >> 5) + 8 * e][tid & 31] = rb[e];
            } else {
                As[tid & 63][4 * e + (tid >> 6)] = ra[e];
                Bs[tid & 63][4 * e + (tid >> 6)] = rb[e];
            }
        }
    };

    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    load(0);
    for (int k0 = 0; k0 < g.K; k0 += 32) {
        __syncthreads();
        store();
        __syncthreads();
        if (k0 + 32 < g.K) load(k0 + 32);
        mma_step<T>(acc, As, Bs, wm, wn, lane);
    }

    const int r = lane & 15, q = lane >> 4;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int m = m0 + wm + i * 16 + 4 * q + v, n = n0 + wn + j * 16 + r;
                if (m >= g.M || n >= g.N) continue;
                const float x = acc[i][j][v];
                if (MODE == DGRAD) {
                    g.c[(size_t)m * g.N + n] = x;
                } else if (n < 9 * g.c_in) {
                    float* o = g.c + (size_t)m * 9 * g.c_in + n;
                    *o = g.accumulate ? *o + x : x;
                } else {
                    float* o = g.db + m;
                    *o = g.accumulate ? *o + x : x;
                }
            }
}

// ------------------------------------------------------------------ CubePad(1) adjoint
// dx[img, p, n] = mask * sum over the padded positions whose CubePad source is p (inverse table, ascending order) of
// dxpad[cube, position, n];  mask = (act[img, p, act_coff + n] > 0) when act is given (ReLU of the saved activation).
template <typename TA, typename TO>
__global__ __launch_bounds__(256) void cubepad_adjoint_kernel(const float* __restrict__ dxpad, const int* __restrict__ off,
                                                              const int* __restrict__ ent, int n_img, int face, int N,
                                                              const TA* __restrict__ act, int act_ld, int act_coff,
                                                              TO* __restrict__ dx, int accumulate) {
    const int fsq = face * face, fp2 = (face + 2) * (face + 2);
    const long long total = (long long)n_img * fsq * N;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        const long long pix = idx / N;
        const int n = (int)(idx - pix * N);
        const int img = (int)(pix / fsq), p = (int)(pix - (long long)img * fsq), f = img % 6;
        const int q = f * fsq + p;
        const float* base = dxpad + (size_t)(img - f) * fp2 * N + n;
        float s = 0.f;
        for (int e = off[q]; e < off[q + 1]; ++e) s += base[(size_t)ent[e] * N];
        if (act && !(load_as_f32<TA>(act + (size_t)pix * act_ld + act_coff + n) > 0.f)) s = 0.f;
        TO* o = dx + (size_t)pix * N + n;
        if (accumulate) *o = from_f32<TO>(load_as_f32<TO>(o) + s);
        else *o = from_f32<TO>(s);
    }
}

// ------------------------------------------------------------------ saliency (to_equi_nn + channel max) and its backward
// One wave per output pixel; the bilinear taps exactly as cube2equi_kernel (projection.hip).  Ties: the lowest channel.
__global__ __launch_bounds__(256) void sal_forward_kernel(const float* __restrict__ h, const int8_t* __restrict__ face_map,
                                                          const float2* __restrict__ coord, float* __restrict__ out_max,
                                                          int* __restrict__ argmax, int B, int C, int w) {
    const int npix = 8 * w * w;
    const int lane = threadIdx.x & 63;
    const int wave_global = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wave_global >= B * npix) return;
    const int b = wave_global / npix, pix = wave_global - b * npix;
    const int f = face_map[pix];
    const float2 pc = coord[pix];
    const float flx = floorf(pc.x), fly = floorf(pc.y);
    const int x0 = (int)flx, y0 = (int)fly;
    const float fx = pc.x - flx, fy = pc.y - fly;
    const float wt[4] = {(1.f - fx) * (1.f - fy), fx * (1.f - fy), (1.f - fx) * fy, fx * fy};
    const int xs[4] = {x0, x0 + 1, x0, x0 + 1}, ys[4] = {y0, y0, y0 + 1, y0 + 1};
    bool ok[4];
    size_t off[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        ok[k] = xs[k] >= 0 && xs[k] < w && ys[k] >= 0 && ys[k] < w;
        const int yy = ok[k] ? ys[k] : 0, xx = ok[k] ? xs[k] : 0;
        off[k] = (((size_t)(b * 6 + f) * w + yy) * w + xx) * C;
    }
    float best = -INFINITY;
    int bi = C;
    for (int c = lane; c < C; c += 64) {
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float v = ok[k] ? h[off[k] + c] : 0.f;
            acc += v * wt[k];
        }
        if (acc > best) { best = acc; bi = c; }       // strict: the first maximum of this lane's channels
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    if (lane == 0) {
        out_max[(size_t)b * npix + pix] = best;
        argmax[(size_t)b * npix + pix] = bi < C ? bi : 0;
    }
}

// One thread per (clip, cube pixel): the (equirectangular pixel, tap) pairs that sample it, in ascending order.
__global__ __launch_bounds__(256) void sal_backward_kernel(const float* __restrict__ dmap, const int* __restrict__ argmax,
                                                           const float2* __restrict__ coord, const int* __restrict__ off,
                                                           const int* __restrict__ ent, float* __restrict__ dh, int B, int C,
                                                           int w) {
    const int npix = 8 * w * w, ncube = 6 * w * w;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * ncube) return;
    const int b = idx / ncube, q = idx - b * ncube;
    for (int e = off[q]; e < off[q + 1]; ++e) {
        const int pix = ent[e] >> 2, k = ent[e] & 3;
        const float2 pc = coord[pix];
        const float fx = pc.x - floorf(pc.x), fy = pc.y - floorf(pc.y);
        const float wt = k == 0 ? (1.f - fx) * (1.f - fy) : (k == 1 ? fx * (1.f - fy) : (k == 2 ? (1.f - fx) * fy : fx * fy));
        const int c = argmax[(size_t)b * npix + pix];
        dh[((size_t)b * ncube + q) * C + c] += dmap[(size_t)b * npix + pix] * wt;
    }
}

unsigned grid_of(long long total) {
    long long blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    return (unsigned)(blocks > 0 ? blocks : 1);
}

}  // namespace

// ================================================================== C ABI (include/cp360.h, "K5t")
extern "C" int cp360_train_gates(const float* gates_partial, int splits, const float* bias, const float* c_prev,
                                 float* c_next, void* h_out, int h_dtype, int ld_h, int h_coff, float* h_f32, float* acts,
                                 int M, int Hc, void* stream) {
    if (!gates_partial || !bias || !c_prev || !c_next || !h_out || !acts) return CP360_ERR_NULL;
    if (splits < 1 || M <= 0 || Hc <= 0 || h_coff < 0 || h_coff + Hc > ld_h) return CP360_ERR_BAD_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    const unsigned blocks = grid_of((long long)M * Hc);
    if (h_dtype == CP360_F32)
        hipLaunchKernelGGL((train_gates_kernel<float>), dim3(blocks), dim3(256), 0, st, gates_partial, splits, bias, c_prev,
                           c_next, (float*)h_out, ld_h, h_coff, h_f32, acts, M, Hc);
    else if (h_dtype == CP360_BF16)
        hipLaunchKernelGGL((train_gates_kernel<bf16_raw>), dim3(blocks), dim3(256), 0, st, gates_partial, splits, bias, c_prev,
                           c_next, (bf16_raw*)h_out, ld_h, h_coff, h_f32, acts, M, Hc);
    else
        return CP360_ERR_BAD_DTYPE;
    CP360_CHECK_HIP();
    return CP360_OK;
}

extern "C" int cp360_train_gates_backward(const float* dh, float* dc, const float* acts, const float* c_prev,
                                          const float* c_next, void* dgates, int dg_dtype, int M, int Hc, void* stream) {
    if (!dh || !dc || !acts || !c_prev || !c_next || !dgates) return CP360_ERR_NULL;
    if (M <= 0 || Hc <= 0) return CP360_ERR_BAD_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    const unsigned blocks = grid_of((long long)M * Hc);
    if (dg_dtype == CP360_F32)
        hipLaunchKernelGGL((train_gates_bwd_kernel<float>), dim3(blocks), dim3(256), 0, st, dh, dc, acts, c_prev, c_next,
                           (float*)dgates, M, Hc);
    else if (dg_dtype == CP360_BF16)
        hipLaunchKernelGGL((train_gates_bwd_kernel<bf16_raw>), dim3(blocks), dim3(256), 0, st, dh, dc, acts, c_prev, c_next,
                           (bf16_raw*)dgates, M, Hc);
    else
        return CP360_ERR_BAD_DTYPE;
    CP360_CHECK_HIP();
    return CP360_OK;
}

extern "C" size_t cp360_train_dgrad_packed_bytes(int dtype, int c_out, int n) {
    if (c_out <= 0 || n <= 0) return 0;
    if (dtype == CP360_F32) return (size_t)n * 9 * c_out * 4;
    if (dtype == CP360_BF16) return (size_t)n * 9 * c_out * 2;
    return 0;
}

extern "C" int cp360_train_dgrad_pack(int dtype, const float* w, int c_out, int c_in, int ci0, int n, void* packed,
                                      void* stream) {
    if (!w || !packed) return CP360_ERR_NULL;
    if (c_out <= 0 || c_in <= 0 || n <= 0 || ci0 < 0 || ci0 + n > c_in) return CP360_ERR_BAD_SHAPE;
    if ((long long)n * 9 * c_out >= (1LL << 31)) return CP360_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((n + 31) / 32, (c_out + 31) / 32);
    if (dtype == CP360_F32)
        hipLaunchKernelGGL((dgrad_pack_kernel<float>), grid, dim3(256), 0, st, w, (float*)packed, c_out, c_in, ci0, n);
    else if (dtype == CP360_BF16)
        hipLaunchKernelGGL((dgrad_pack_kernel<bf16_raw>), grid, dim3(256), 0, st, w, (bf16_raw*)packed, c_out, c_in, ci0, n);
    else
        return CP360_ERR_BAD_DTYPE;
    CP360_CHECK_HIP();
    return CP360_OK;
}

extern "C" int cp360_train_dgrad(int dtype, const void* dy, int n_img, int face, int c_out, const void* packed, int n,
                                 float* dxpad, void* stream) {
    if (!dy || !packed || !dxpad) return CP360_ERR_NULL;
    if (n_img <= 0 || face <= 0 || c_out <= 0 || n <= 0) return CP360_ERR_BAD_SHAPE;
    if (n_img % 6) return CP360_ERR_BATCH_NOT_6N;
    const long long M = (long long)n_img * (face + 2) * (face + 2);
    if (M * n >= (1LL << 31) || (long long)n * 9 * c_out >= (1LL << 31) || (long long)n_img * face * face * c_out >= (1LL << 31))
        return CP360_ERR_UNSUPPORTED;
    GemmArgs g{dy, packed, nullptr, dxpad, nullptr, (int)M, n, 9 * c_out, face, c_out, 0, 0, 0};
    const dim3 grid((n + 63) / 64, (unsigned)((M + 63) / 64));
    hipStream_t st = (hipStream_t)stream;
    if (dtype == CP360_F32) hipLaunchKernelGGL((train_gemm_kernel<float, DGRAD>), grid, dim3(256), 0, st, g);
    else if (dtype == CP360_BF16) hipLaunchKernelGGL((train_gemm_kernel<bf16_raw, DGRAD>), grid, dim3(256), 0, st, g);
    else return CP360_ERR_BAD_DTYPE;
    CP360_CHECK_HIP();
    return CP360_OK;
}

extern "C" int cp360_train_cubepad_inverse_host(int face, int32_t* offsets, int32_t* entries) {
    if (!offsets || !entries) return CP360_ERR_NULL;
    if (face <= 0) return CP360_ERR_BAD_SHAPE;
    const CubePadGeom geo{face, 1, 1, 1, 1};
    const int fp = face + 2, ncube = 6 * face * face, npad = 6 * fp * fp;
    std::vector<int> src(npad), cnt(ncube + 1, 0);
    for (int f = 0; f < 6; ++f)
        for (int i = 0; i < fp; ++i)
            for (int j = 0; j < fp; ++j) {
                const int r = (f * fp + i) * fp + j;
                src[r] = cubepad_src(f, i, j, geo);
                ++cnt[src[r] + 1];
            }
    offsets[0] = 0;
    for (int q = 0; q < ncube; ++q) offsets[q + 1] = offsets[q] + cnt[q + 1];
    std::vector<int> fill(offsets, offsets + ncube);
    for (int r = 0; r < npad; ++r) entries[fill[src[r]]++] = r;          // ascending padded position per source
    return CP360_OK;
}

extern "C" int cp360_train_cubepad_adjoint(const float* dxpad, const int32_t* offsets, const int32_t* entries, int n_img,
                                           int face, int n, const void* act, int act_dtype, int act_ld, int act_coff,
                                           void* dx, int dx_dtype, int accumulate, void* stream) {
    if (!dxpad || !offsets || !entries || !dx) return CP360_ERR_NULL;
    if (n_img <= 0 || face <= 0 || n <= 0 || (act && (act_coff < 0 || act_coff + n > act_ld))) return CP360_ERR_BAD_SHAPE;
    if (n_img % 6) return CP360_ERR_BATCH_NOT_6N;
    if (act && act_dtype != dx_dtype && act_dtype != CP360_F32) return CP360_ERR_BAD_DTYPE;
    hipStream_t st = (hipStream_t)stream;
    const unsigned blocks = grid_of((long long)n_img * face * face * n);
#define CP360_ADJ(TA, TO)                                                                                                     \
    hipLaunchKernelGGL((cubepad_adjoint_kernel<TA, TO>), dim3(blocks), dim3(256), 0, st, dxpad, offsets, entries, n_img, face, \
                       n, (const TA*)act, act_ld, act_coff, (TO*)dx, accumulate)
    const bool a16 = act && act_dtype == CP360_BF16;
    if (dx_dtype == CP360_F32) {
        if (a16) CP360_ADJ(bf16_raw, float); else CP360_ADJ(float, float);
    } else if (dx_dtype == CP360_BF16) {
        if (a16) CP360_ADJ(bf16_raw, bf16_raw); else CP360_ADJ(float, bf16_raw);
    } else {
        return CP360_ERR_BAD_DTYPE;
    }
#undef CP360_ADJ
    CP360_CHECK_HIP();
    return CP360_OK;
}

extern "C" int cp360_train_wgrad(int dtype, const void* dy, const void* x, int ldx, const int32_t* pad_table, int n_img,
                                 int face, int c_out, int c_in, float* dw, float* db, int accumulate, void* stream) {
    if (!dy || !x || !pad_table || !dw) return CP360_ERR_NULL;
    if (n_img <= 0 || face <= 0 || c_out <= 0 || c_in <= 0 || ldx < c_in) return CP360_ERR_BAD_SHAPE;
    if (n_img % 6) return CP360_ERR_BATCH_NOT_6N;
    const long long K = (long long)n_img * face * face, N = 9LL * c_in + (db ? 1 : 0);
    if (K * ldx >= (1LL << 31) || K * c_out >= (1LL << 31) || (long long)c_out * N >= (1LL << 31)) return CP360_ERR_UNSUPPORTED;
    GemmArgs g{dy, x, pad_table, dw, db, c_out, (int)N, (int)K, face, c_out, c_in, ldx, accumulate ? 1 : 0};
    const dim3 grid((unsigned)((N + 63) / 64), (c_out + 63) / 64);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == CP360_F32) hipLaunchKernelGGL((train_gemm_kernel<float, WGRAD>), grid, dim3(256), 0, st, g);
    else if (dtype == CP360_BF16) hipLaunchKernelGGL((train_gemm_kernel<bf16_raw, WGRAD>), grid, dim3(256), 0, st, g);
    else return CP360_ERR_BAD_DTYPE;
    CP360_CHECK_HIP();
    return CP360_OK;
}

extern "C" int cp360_train_c2e_inverse_host(const int8_t* face_map, const float* coord, int w, int32_t* offsets,
                                            int32_t* entries) {
    if (!face_map || !coord || !offsets || !entries) return CP360_ERR_NULL;
    if (w <= 0) return CP360_ERR_BAD_SHAPE;
    const int npix = 8 * w * w, ncube = 6 * w * w;
    std::vector<int> tgt(4 * npix, -1), cnt(ncube + 1, 0);
    for (int pix = 0; pix < npix; ++pix) {
        const int f = face_map[pix];
        if (f < 0 || f > 5) return CP360_ERR_BAD_SHAPE;
        const int x0 = (int)floorf(coord[2 * pix]), y0 = (int)floorf(coord[2 * pix + 1]);
        for (int k = 0; k < 4; ++k) {
            const int xx = x0 + (k & 1), yy = y0 + (k >> 1);
            if (xx < 0 || xx >= w || yy < 0 || yy >= w) continue;
            tgt[4 * pix + k] = (f * w + yy) * w + xx;
            ++cnt[tgt[4 * pix + k] + 1];
        }
    }
    offsets[0] = 0;
    for (int q = 0; q < ncube; ++q) offsets[q + 1] = offsets[q] + cnt[q + 1];
    std::vector<int> fill(offsets, offsets + ncube);
    for (int e = 0; e < 4 * npix; ++e)
        if (tgt[e] >= 0) entries[fill[tgt[e]]++] = e;                   // (pixel << 2 | tap), ascending
    return offsets[ncube];
}

extern "C" int cp360_train_saliency_forward(const float* h, const int8_t* face_map, const float* coord, float* out_max,
                                            int32_t* argmax, int B, int C, int w, void* stream) {
    if (!h || !face_map || !coord || !out_max || !argmax) return CP360_ERR_NULL;
    if (B <= 0 || C <= 0 || w <= 0) return CP360_ERR_BAD_SHAPE;
    const int waves = B * 8 * w * w;
    hipLaunchKernelGGL(sal_forward_kernel, dim3((waves + 3) / 4), dim3(256), 0, (hipStream_t)stream, h, face_map,
                       (const float2*)coord, out_max, argmax, B, C, w);
    CP360_CHECK_HIP();
    return CP360_OK;
}

extern "C" int cp360_train_saliency_backward(const float* dmap, const int32_t* argmax, const float* coord,
                                             const int32_t* offsets, const int32_t* entries, float* dh, int B, int C, int w,
                                             void* stream) {
    if (!dmap || !argmax || !coord || !offsets || !entries || !dh) return CP360_ERR_NULL;
    if (B <= 0 || C <= 0 || w <= 0) return CP360_ERR_BAD_SHAPE;
    const int threads = B * 6 * w * w;
    hipLaunchKernelGGL(sal_backward_kernel, dim3((threads + 255) / 256), dim3(256), 0, (hipStream_t)stream, dmap, argmax,
                       (const float2*)coord, offsets, entries, dh, B, C, w);
    CP360_CHECK_HIP();
    return CP360_OK;
}
