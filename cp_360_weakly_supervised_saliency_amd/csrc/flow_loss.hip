// K5f: flow resize and flow loss (temporal_model/train_temporal.py:110-167 of the reference).
//
// Flow resize: cv2.resize(flow, (2 flow_h, flow_h), interpolation=cv2.INTER_CUBIC) of every flow the loss reads, multiplied by
// fscale = flow_h / W_in afterwards (the reference divides by the WIDTH).  OpenCV's generic float path:
//   inv_scale = (double)dst / src, scale = 1.0 / inv_scale;
//   f = (float)((d + 0.5) * scale - 0.5), s = floor(f), f -= s;
//   A = -0.75f, in float:  c0 = ((A (f+1) - 5A)(f+1) + 8A)(f+1) - 4A,  c1 = ((A+2) f - (A+3)) f^2 + 1,
//                          c2 = ((A+2)(1-f) - (A+3))(1-f)^2 + 1,      c3 = 1 - c0 - c1 - c2;
//   taps s-1 .. s+2 clamped to [0, n-1] (replicate), horizontal pass first, then vertical, both accumulated in f32.
// Equal sizes: cv2 copies the input, so only the scale is applied.  The per-axis tables are built on the host
// (cp360_flow_resize_coeffs_host) and uploaded by the caller; the kernel gathers 4 x 4 taps per output pixel (HBM-bound).
//
// Flow loss: the three sum-MSE terms of all B x L pairs (map fidx -> map fidx + 1 of each clip) in one launch sequence,
// restating torch's CPU semantics:
//   upsample   F.interpolate(bilinear, align_corners=False) of a 2w x 4w map to (H, W):
//              src = max((dst + 0.5) * in / out - 0.5, 0), upper neighbour clamped to in - 1;
//   warp       grid_sample(bilinear, zeros, align_corners=False) of the UPSAMPLED current map at
//              grid = flow / (W, H) * 2 + mesh (mesh on the (size - 1) grid), ix = ((gx + 1) W - 1) / 2; each of the 4 corners
//              is itself a bilinear tap of the small map (staged in LDS), so no upsampled map ever reaches HBM;
//   mask       static = sqrt(fx^2 + fy^2) < mm_th on the scaled flow;
//   terms      sm += (next - warp)^2, temp += (next - cur)^2, mask += static ? next^2 : 0.
// The gradient reaches only the next map of each pair (warp, cur and the mask target are detached):
//   d_up = 2 (g_sm (next - warp) + g_t (next - cur) + g_m static next), then the adjoint of the separable upsample onto map
//   fidx + 1: R[y][j] = sum_x d_up[y][x] wx(x, j) per loss row, dmap[i][j] = sum_y wy(y, i) R[y][j]; map 0 gets zero.
// No atomics and no schedule-dependent order anywhere: the loss partial sums go per workgroup to the work buffer and are
// reduced in a fixed order, every gradient element is a fixed-order sum.  The backward pass recomputes the per-pixel residuals
// from the maps and the flow, so the forward stores nothing per pixel.
//
//   flow_resize_kernel      [F, H_in, W_in, 2] -> [F, H_out, W_out, 2] * fscale (4 x 4 taps, or the scale alone)
//   flow_loss_fwd_kernel    per (pair, 2048 pixels): the three partial sums
//   flow_loss_reduce_kernel the partial sums of all workgroups, in order, in double -> loss[3]
//   flow_loss_rows_kernel   per (pair, loss row): d_up of the row, then R[pair][y][0 .. 4w)
//   flow_loss_cols_kernel   per map pixel: dmap = sum over the loss rows of wy * R (zero for map 0 of each clip)
#include "common.h"
#include "../../include/cp360.h"

#include <math.h>

namespace {

constexpr int kMaxMapFloats = 2048;      // 2w x 4w at w <= 16
constexpr int kFwdPixels = 2048;         // loss pixels per forward workgroup (256 threads x 8)
constexpr int kRowChunk = 1024;          // d_up values of one loss row staged at a time by the backward row kernel

// ------------------------------------------------------------------ resize
__global__ __launch_bounds__(256) void flow_resize_kernel(const float2* __restrict__ in, float2* __restrict__ out, int F,
                                                          int hi, int wi, int ho, int wo, const int32_t* __restrict__ yofs,
                                                          const float4* __restrict__ ycoef, const int32_t* __restrict__ xofs,
                                                          const float4* __restrict__ xcoef, float fscale) {
    const long long total = (long long)F * ho * wo;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        if (!yofs) {                                  // equal sizes: cv2 copies, the reference scales
            const float2 v = in[idx];
            out[idx] = make_float2(fscale * v.x, fscale * v.y);
            continue;
        }
        const int x = (int)(idx % wo);
        const long long t = idx / wo;
        const int y = (int)(t % ho), f = (int)(t / ho);
        const int sx = xofs[x], sy = yofs[y];
        const float4 cx = xcoef[x], cy = ycoef[y];
        int xs[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) xs[k] = min(max(sx - 1 + k, 0), wi - 1);
        const float cyk[4] = {cy.x, cy.y, cy.z, cy.w};
        float ax = 0.f, ay = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int yy = min(max(sy - 1 + r, 0), hi - 1);
            const float2* row = in + ((size_t)f * hi + yy) * wi;
            const float2 p0 = row[xs[0]], p1 = row[xs[1]], p2 = row[xs[2]], p3 = row[xs[3]];
            const float hx = p0.x * cx.x + p1.x * cx.y + p2.x * cx.z + p3.x * cx.w;
            const float hy = p0.y * cx.x + p1.y * cx.y + p2.y * cx.z + p3.y * cx.w;
            ax += hx * cyk[r];
            ay += hy * cyk[r];
        }
        out[idx] = make_float2(fscale * ax, fscale * ay);
    }
}

// ------------------------------------------------------------------ loss
// One axis of torch's bilinear upsample (align_corners=False, CPU): source index, its upper neighbour's offset, the lambdas.
struct Tap {
    int i0, p;
    float l0, l1;
};

__device__ __forceinline__ Tap up_tap(int dst, int in, float scale) {
    float src = scale * ((float)dst + 0.5f) - 0.5f;
    src = fmaxf(src, 0.f);
    Tap t;
    t.i0 = min((int)floorf(src), in - 1);
    t.l1 = fminf(fmaxf(src - (float)t.i0, 0.f), 1.f);
    t.l0 = 1.f - t.l1;
    t.p = t.i0 < in - 1 ? 1 : 0;
    return t;
}

// the upsampled value at (ty, tx) of a small map m [*, ld] in LDS
__device__ __forceinline__ float up_val(const float* m, int ld, Tap ty, Tap tx) {
    const float* r0 = m + ty.i0 * ld + tx.i0;
    const float* r1 = r0 + ty.p * ld;
    return ty.l0 * (tx.l0 * r0[0] + tx.l1 * r0[tx.p]) + ty.l1 * (tx.l0 * r1[0] + tx.l1 * r1[tx.p]);
}

struct Residual {
    float next, d_warp, d_cur;
    bool stat;
};

// The per-pixel quantities of one pair at loss pixel (y, x): cur / next small maps in LDS (2w x 4w), scaled flow (fx, fy).
__device__ __forceinline__ Residual residual(const float* sc, const float* sn, int mh, int mw, int h, int wl, int y, int x,
                                            float2 fl, float mm_th, float scy, float scx) {
    const Tap ty = up_tap(y, mh, scy), tx = up_tap(x, mw, scx);
    Residual r;
    r.next = up_val(sn, mw, ty, tx);
    const float cur = up_val(sc, mw, ty, tx);
    r.stat = sqrtf(__fadd_rn(__fmul_rn(fl.x, fl.x), __fmul_rn(fl.y, fl.y))) < mm_th;
    // grid = flow / size * 2 + mesh, mesh = i / (size - 1) * 2 - 1; unnormalised as grid_sample(align_corners=False)
    const float gx = fl.x / (float)wl * 2.f + ((float)x / (float)(wl - 1) * 2.f - 1.f);
    const float gy = fl.y / (float)h * 2.f + ((float)y / (float)(h - 1) * 2.f - 1.f);
    // clamped so that far-out samples (every corner outside: zero) keep their integer corners in range
    const float ix = fminf(fmaxf(((gx + 1.f) * (float)wl - 1.f) / 2.f, -2.f), (float)wl + 1.f);
    const float iy = fminf(fmaxf(((gy + 1.f) * (float)h - 1.f) / 2.f, -2.f), (float)h + 1.f);
    const float fx0 = floorf(ix), fy0 = floorf(iy);
    const int x0 = (int)fx0, y0 = (int)fy0;
    const float wx1 = ix - fx0, wx0 = (fx0 + 1.f) - ix;
    const float wy1 = iy - fy0, wy0 = (fy0 + 1.f) - iy;
    const bool vx0 = x0 >= 0 && x0 < wl, vx1 = x0 + 1 >= 0 && x0 + 1 < wl;
    const bool vy0 = y0 >= 0 && y0 < h, vy1 = y0 + 1 >= 0 && y0 + 1 < h;
    float warp = 0.f;
    if (vy0 || vy1) {
        Tap cx0, cx1;
        if (vx0) cx0 = up_tap(x0, mw, scx);
        if (vx1) cx1 = up_tap(x0 + 1, mw, scx);
        if (vy0) {
            const Tap cy = up_tap(y0, mh, scy);
            if (vx0) warp += up_val(sc, mw, cy, cx0) * (wx0 * wy0);
            if (vx1) warp += up_val(sc, mw, cy, cx1) * (wx1 * wy0);
        }
        if (vy1) {
            const Tap cy = up_tap(y0 + 1, mh, scy);
            if (vx0) warp += up_val(sc, mw, cy, cx0) * (wx0 * wy1);
            if (vx1) warp += up_val(sc, mw, cy, cx1) * (wx1 * wy1);
        }
    }
    r.d_warp = r.next - warp;
    r.d_cur = r.next - cur;
    return r;
}

__device__ __forceinline__ void stage_maps(const float* __restrict__ maps, int L, int ms, int pair, float* sc, float* sn) {
    const int b = pair / L, f = pair - b * L;
    const float* cur = maps + ((size_t)b * (L + 1) + f) * ms;
    for (int i = threadIdx.x; i < ms; i += blockDim.x) {
        sc[i] = cur[i];
        sn[i] = cur[ms + i];
    }
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(256) void flow_loss_fwd_kernel(const float* __restrict__ maps, const float2* __restrict__ flow,
                                                            int L, int w, int h, int wl, float mm_th,
                                                            float* __restrict__ partial) {
    __shared__ float sc[kMaxMapFloats], sn[kMaxMapFloats];
    __shared__ float red[4][3];
    const int pair = blockIdx.y, mh = 2 * w, mw = 4 * w;
    stage_maps(maps, L, mh * mw, pair, sc, sn);
    __syncthreads();
    const float scy = (float)mh / (float)h, scx = (float)mw / (float)wl;
    const long long hw = (long long)h * wl;
    const float2* fp = flow + (size_t)pair * hw;
    float a_sm = 0.f, a_t = 0.f, a_m = 0.f;
    const long long base = (long long)blockIdx.x * kFwdPixels;
#pragma unroll 2
    for (int k = 0; k < kFwdPixels / 256; ++k) {
        const long long px = base + k * 256 + threadIdx.x;
        if (px < hw) {
            const int y = (int)(px / wl), x = (int)(px - (long long)y * wl);
            const Residual r = residual(sc, sn, mh, mw, h, wl, y, x, fp[px], mm_th, scy, scx);
            a_sm += r.d_warp * r.d_warp;
            a_t += r.d_cur * r.d_cur;
            a_m += r.stat ? r.next * r.next : 0.f;
        }
    }
    a_sm = wave_sum(a_sm);
    a_t = wave_sum(a_t);
    a_m = wave_sum(a_m);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[wave][0] = a_sm;
        red[wave][1] = a_t;
        red[wave][2] = a_m;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int t = threadIdx.x;
        partial[((size_t)pair * gridDim.x + blockIdx.x) * 3 + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
    }
}

__global__ __launch_bounds__(256) void flow_loss_reduce_kernel(const float* __restrict__ partial, int n, float* __restrict__ loss) {
    __shared__ double red[3][256];
    double a[3] = {0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < n; i += 256) {
#pragma unroll
        for (int t = 0; t < 3; ++t) a[t] += (double)partial[(size_t)i * 3 + t];
    }
#pragma unroll
    for (int t = 0; t < 3; ++t) red[t][threadIdx.x] = a[t];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
#pragma unroll
            for (int t = 0; t < 3; ++t) red[t][threadIdx.x] += red[t][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x < 3) loss[threadIdx.x] = (float)red[threadIdx.x][0];
}

// The first destination index whose upsample source index i0 is >= target (i0 is non-decreasing in the destination index).
__device__ __forceinline__ int first_at_least(int target, int out, int in, float scale) {
    int lo = 0, hi = out;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (up_tap(mid, in, scale).i0 >= target) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// the weight of source index j in the upsample of destination index d
__device__ __forceinline__ float up_weight(int d, int j, int in, float scale) {
    const Tap t = up_tap(d, in, scale);
    return (t.i0 == j ? t.l0 : 0.f) + (t.i0 + t.p == j ? t.l1 : 0.f);
}

__global__ __launch_bounds__(256) void flow_loss_rows_kernel(const float* __restrict__ maps, const float2* __restrict__ flow,
                                                             const float* __restrict__ gout, int L, int w, int h, int wl,
                                                             float mm_th, float* __restrict__ R) {
    __shared__ float sc[kMaxMapFloats], sn[kMaxMapFloats];
    __shared__ float dup[kRowChunk];
    __shared__ float part[256];
    const int y = blockIdx.x, pair = blockIdx.y, mh = 2 * w, mw = 4 * w;
    stage_maps(maps, L, mh * mw, pair, sc, sn);
    const float scy = (float)mh / (float)h, scx = (float)mw / (float)wl;
    const float g_sm = gout[0], g_t = gout[1], g_m = gout[2];
    const float2* fp = flow + ((size_t)pair * h + y) * wl;
    // thread (j, s): column j of the small map, s-th of nsub interleaved slices of the loss columns that touch j
    const int nsub = 256 / mw;
    const int j = threadIdx.x / nsub, s = threadIdx.x - j * nsub;
    const bool active = j < mw;
    int lo = 0, hi = 0;
    if (active) {
        lo = first_at_least(j - 1, wl, mw, scx);
        hi = first_at_least(j + 1, wl, mw, scx);
    }
    float acc = 0.f;
    for (int c0 = 0; c0 < wl; c0 += kRowChunk) {
        __syncthreads();                               // maps staged / the previous chunk consumed
        const int n = min(kRowChunk, wl - c0);
        for (int i = threadIdx.x; i < n; i += 256) {
            const int x = c0 + i;
            const Residual r = residual(sc, sn, mh, mw, h, wl, y, x, fp[x], mm_th, scy, scx);
            dup[i] = 2.f * (g_sm * r.d_warp + g_t * r.d_cur + (r.stat ? g_m * r.next : 0.f));
        }
        __syncthreads();
        if (active) {
            const int a = max(lo, c0), e = min(hi, c0 + n);
            for (int x = a + s; x < e; x += nsub) acc += up_weight(x, j, mw, scx) * dup[x - c0];
        }
    }
    part[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x < mw) {
        float v = 0.f;
        for (int q = 0; q < nsub; ++q) v += part[threadIdx.x * nsub + q];
        R[((size_t)pair * h + y) * mw + threadIdx.x] = v;
    }
}

__global__ __launch_bounds__(256) void flow_loss_cols_kernel(const float* __restrict__ R, int B, int L, int w, int h,
                                                             float* __restrict__ dmaps) {
    const int mh = 2 * w, mw = 4 * w, ms = mh * mw;
    const int total = B * (L + 1) * ms;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int m = idx / ms, q = idx - m * ms;
    const int b = m / (L + 1), k = m - b * (L + 1);
    float v = 0.f;
    if (k > 0) {
        const int i = q / mw, j = q - i * mw;
        const float scy = (float)mh / (float)h;
        const int lo = first_at_least(i - 1, h, mh, scy), hi = first_at_least(i + 1, h, mh, scy);
        const float* r = R + (size_t)(b * L + k - 1) * h * mw + j;
        for (int y = lo; y < hi; ++y) v += up_weight(y, i, mh, scy) * r[(size_t)y * mw];
    }
    dmaps[idx] = v;
}

int grid_1d(long long n) {
    long long g = (n + 255) / 256;
    return (int)(g < 65536 ? (g < 1 ? 1 : g) : 65536);
}

int check_loss_args(int dtype, int B, int L, int w, int h, int wl) {
    if (dtype != CP360_F32) return CP360_ERR_BAD_DTYPE;
    if (B <= 0 || L <= 0 || w <= 0 || h < 2 || wl < 2) return CP360_ERR_BAD_SHAPE;
    if (8 * w * w > kMaxMapFloats || h > 65535 || (long long)h * wl > (1LL << 30)) return CP360_ERR_UNSUPPORTED;
    if ((long long)B * L > 65535) return CP360_ERR_UNSUPPORTED;
    return CP360_OK;
}

long long fwd_blocks(int h, int wl) { return ((long long)h * wl + kFwdPixels - 1) / kFwdPixels; }

}  // namespace

// ------------------------------------------------------------------ C ABI
extern "C" int cp360_flow_resize_coeffs_host(int in_size, int out_size, int32_t* ofs, float* coef) {
#pragma clang fp contract(off)
    if (!ofs || !coef) return CP360_ERR_NULL;
    if (in_size <= 0 || out_size <= 0) return CP360_ERR_BAD_SHAPE;
    const double inv_scale = (double)out_size / in_size, scale = 1.0 / inv_scale;
    const float A = -0.75f;
    for (int d = 0; d < out_size; ++d) {
        float f = (float)((d + 0.5) * scale - 0.5);
        const int s = (int)floorf(f);
        f -= (float)s;
        const float c0 = ((A * (f + 1) - 5 * A) * (f + 1) + 8 * A) * (f + 1) - 4 * A;
        const float c1 = ((A + 2) * f - (A + 3)) * f * f + 1;
        const float c2 = ((A + 2) * (1 - f) - (A + 3)) * (1 - f) * (1 - f) + 1;
        const float c3 = 1.f - c0 - c1 - c2;
        ofs[d] = s;
        coef[4 * d] = c0;
        coef[4 * d + 1] = c1;
        coef[4 * d + 2] = c2;
        coef[4 * d + 3] = c3;
    }
    return CP360_OK;
}

extern "C" int cp360_flow_resize(int dtype, const float* flow, int F, int h_in, int w_in, float* out, int h_out, int w_out,
                                 const int32_t* yofs, const float* ycoef, const int32_t* xofs, const float* xcoef,
                                 float fscale, void* stream) {
    if (dtype != CP360_F32) return CP360_ERR_BAD_DTYPE;
    if (!flow || !out) return CP360_ERR_NULL;
    if (F <= 0 || h_in <= 0 || w_in <= 0 || h_out <= 0 || w_out <= 0) return CP360_ERR_BAD_SHAPE;
    const bool same = h_in == h_out && w_in == w_out;
    if (!same && (!yofs || !ycoef || !xofs || !xcoef)) return CP360_ERR_NULL;
    const long long total = (long long)F * h_out * w_out;
    hipLaunchKernelGGL(flow_resize_kernel, dim3(grid_1d(total)), dim3(256), 0, (hipStream_t)stream, (const float2*)flow,
                       (float2*)out, F, h_in, w_in, h_out, w_out, same ? nullptr : yofs, (const float4*)ycoef,
                       same ? nullptr : xofs, (const float4*)xcoef, fscale);
    CP360_CHECK_HIP();
    return CP360_OK;
}

extern "C" size_t cp360_flow_loss_work_bytes(int B, int L, int w, int h, int w_loss) {
    if (check_loss_args(CP360_F32, B, L, w, h, w_loss) != CP360_OK) return 0;
    const size_t pairs = (size_t)B * L;
    const size_t fwd = pairs * (size_t)fwd_blocks(h, w_loss) * 3;
    const size_t bwd = pairs * (size_t)h * 4 * w;
    return sizeof(float) * (fwd > bwd ? fwd : bwd);
}

extern "C" int cp360_flow_loss_forward(int dtype, const float* maps, const float* flow, int B, int L, int w, int h, int w_loss,
                                       float mm_th, float* loss, float* work, void* stream) {
    const int st = check_loss_args(dtype, B, L, w, h, w_loss);
    if (st != CP360_OK) return st;
    if (!maps || !flow || !loss || !work) return CP360_ERR_NULL;
    const int nblk = (int)fwd_blocks(h, w_loss);
    hipLaunchKernelGGL(flow_loss_fwd_kernel, dim3(nblk, B * L), dim3(256), 0, (hipStream_t)stream, maps, (const float2*)flow,
                       L, w, h, w_loss, mm_th, work);
    CP360_CHECK_HIP();
    hipLaunchKernelGGL(flow_loss_reduce_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, work, nblk * B * L, loss);
    CP360_CHECK_HIP();
    return CP360_OK;
}

extern "C" int cp360_flow_loss_backward(int dtype, const float* maps, const float* flow, const float* grad_loss, int B, int L,
                                        int w, int h, int w_loss, float mm_th, float* dmaps, float* work, void* stream) {
    const int st = check_loss_args(dtype, B, L, w, h, w_loss);
    if (st != CP360_OK) return st;
    if (!maps || !flow || !grad_loss || !dmaps || !work) return CP360_ERR_NULL;
    hipLaunchKernelGGL(flow_loss_rows_kernel, dim3(h, B * L), dim3(256), 0, (hipStream_t)stream, maps, (const float2*)flow,
                       grad_loss, L, w, h, w_loss, mm_th, work);
    CP360_CHECK_HIP();
    const int total = B * (L + 1) * 8 * w * w;
    hipLaunchKernelGGL(flow_loss_cols_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, work, B, L, w, h,
                       dmaps);
    CP360_CHECK_HIP();
    return CP360_OK;
}
