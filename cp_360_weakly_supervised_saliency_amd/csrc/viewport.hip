// K12: the viewport pilot - a saliency map turned into a camera: the perspective (gnomonic) view of an equirectangular frame
// under a camera rotation (K12a), the view's frame drawn on the panorama (K12b), the saliency map smoothed on the sphere (K12c)
// and its peak with one mean-shift step (K12d); and the camera path that collects the most saliency under a turn limit and a turn
// cost, by dynamic programming over the map's pixels (K16a - K16c); and several cameras at once: the caps about earlier cameras
// taken out of a map (K20a) and several views on one canvas (K20b); and the view anti-aliased by supersampling (K21); and zoom:
// the view and its frame with a lens per frame (K22a, K22b) and how wide the target is (K22d).  The
// reference's utils/fov_visual.py (box_proh, fov_module, draw_cube_fov_box) has this purpose and does not compile; the
// specification is the package's own, DESIGN.md "K12", "K16", "K20", "K21" and "K22"; tests/viewport_restate.py restates K12 in
// float64, tests/campath_restate.py K16 in integers, tests/director_restate.py K20, tests/viewport_aa_restate.py K21,
// tests/zoom_restate.py K22.  Geometry, tables and the bilinear sample are sphere.h's, and so are the view-frame terms of K12b
// and the two sources of a lens: the view (K12a, K21, K22a) and its frame (K12b, K22b) are one kernel template each, which asks
// its source for the lens of a frame - one lens by value for the scalar entry points, K22's table for the _zoom ones.
//
// Camera: R f32 [N, 3, 3] row-major, camera-to-world, columns (forward, up, right).  R = I looks along dir of the panorama's
// centre (1, 0, 0) with up +y and right +z.  tx = tan(hfov / 2), ty = tx h / w (double on the host, rounded to f32 once).
//   K12a  view pixel (i, j): u = ((2 i + 1) / w - 1) tx, v = (1 - (2 j + 1) / h) ty, r = 1 / sqrtf((1 + v v) + u u),
//         d = (r, v r, u r), q = R d, out = bilinear(frame, pix(q)): columns wrap, rows clamp
//   K12b  panorama pixel (x, y): p = dir(x, y), d = R^T p = (d_f, d_u, d_r), u = d_r / d_f, v = d_u / d_f, b = border_px 2 tx / w;
//         border <=> d_f > 0, |u| <= tx, |v| <= ty and not (|u| <= tx - b and |v| <= ty - b)
//   K12c  out_i = sum_j a_j s_j e_ij / sum_j a_j e_ij, e_ij = expf(kappa (p_i . p_j - 1)), kappa = 1 / sigma^2, a_j = cos phi_j
//   K12d  idx = argmax of the smoothed map (lowest index on ties), p* = dir(idx), c = sum_j a_j s_j e(p*, p_j) p_j, dir = c / |c|
//   K16a  q[t][j] = (int)rintf(min(max(s[t][j] g[t], 0), 4096)), 0 where the product is not finite; acc[lo] = q[lo],
//         acc[t][j] = q[t][j] + max_i (acc[t-1][i] - cost(i, j)) over the allowed i, back[t][j] = that i (lowest on ties)
//   K16b  idx[hi-1] = argmax acc[hi-1] (lowest on ties), idx[t-1] = back[t][idx[t]], dir = dir(idx), score = acc[hi-1][idx[hi-1]]
//   K16c  K12d's mean-shift step about p* = dir(idx[t]) for given indices
//   K20a  out[t][j] = +0 where ((p_x d_x + p_y d_y) + p_z d_z) >= (float)cos(radius) for any finite direction d of frame t, else
//         the input's bits
//   K20b  canvas pixel (x0_k + i, y0_k + j) of tile k = K12a's view pixel (i, j) of the view (h_k, w_k, hfov_k) under R[n][k];
//         fill outside every tile and in the tile of a non-finite camera
//   K21   view pixel (i, j) with the factor n = 1 .. 4: s = the n n unrounded f32 samples (n i + a, n j + b) of K12a's view
//         (n h, n w, tx, ty) under R, added in f32 with b outer and a inner from the first sample; out = s / (float)(n n), stored
//         as K12a stores (u8: rintf, clamp).  n = 1 is K12a.  K20b's tiles have a factor each
//   K22   lens f32 [N, 4] = (tx, ty, b, 0) per frame: K22a is K12a / K21 and K22b is K12b with frame n's lens (and factor), bit for
//         bit.  K22d: in_j = ((p_x d_x + p_y d_y) + p_z d_z) >= (float)cos(window), top = max of the finite s_j in the cap,
//         m_j = a_j fmaxf(s_j - (float)level top, 0), g_j = (((p_x - d_x)^2 + (p_y - d_y)^2) + (p_z - d_z)^2) / 2,
//         q = sum m_j g_j / sum m_j
// Every per-pixel term is f32 with plain operators and contraction off; the sums of K12c / K12d / K16c / K22d are f64 in a fixed
// order; K16a / K16b are integers.  No atomics, no host synchronisation, results independent of the batch size.
#pragma clang fp contract(off)

#include "sphere.h"

#include <atomic>

namespace {

constexpr int kMaxMapPx = 16384;             // K12c is all pairs: P^2 terms per frame

// K12d's argmax, one step of its tree (the tree of sphere.h's ordered sum): the candidate (ov, oi) replaces (best, bi) when it
// has the larger value, or the same value at a lower index; an index below 0 is no candidate
template <typename V>
__device__ __forceinline__ void peak_take(V ov, int oi, V& best, int& bi) {
    if (oi >= 0 && (bi < 0 || ov > best || (ov == best && oi < bi))) {
        best = ov;
        bi = oi;
    }
}

// ------------------------------------------------------------------ K12a: the view
// K12a's position: where view pixel (i, j) of the view (h, w, tx, ty) under R lies on the H x W panorama
__device__ __forceinline__ void view_pos(const Rot& R, int H, int W, int h, int w, float tx, float ty, int i, int j, float& sx,
                                         float& sy) {
    const float u = ((float)(2 * i + 1) / (float)w - 1.f) * tx;
    const float v = (1.f - (float)(2 * j + 1) / (float)h) * ty;
    const float r = 1.f / sqrtf((1.f + v * v) + u * u);
    float qx, qy, qz;
    stab_rotate(R, r, v * r, u * r, qx, qy, qz);
    stab_pix(qx, qy, qz, 0.5f * (float)W, 0.5f * (float)H, sx, sy);
}

// K12a's pixel, which K20b repeats per tile: view pixel (i, j) of the view (h, w, tx, ty) under R, sampled from the H x W frame
// `img` into the C channels at o
template <typename T, int C>
__device__ __forceinline__ void view_pixel(const T* __restrict__ img, const Rot& R, int H, int W, int h, int w, float tx, float ty,
                                           int i, int j, T* __restrict__ o) {
    float sx, sy;
    view_pos(R, H, W, h, w, tx, ty, i, j, sx, sy);
    sphere_sample<T, C>(img, H, W, sx, sy, o);
}

// K21's pixel: the NS x NS box mean of the unrounded samples (NS i + a, NS j + b) of the fine view (NS h, NS w, tx, ty) - K12a's
// positions with the fine view's indices and sizes -, added in f32 with b outer and a inner from the first sample, divided by
// (float)(NS NS) and stored as K12a stores.  C accumulators; both loops unrolled.
template <typename T, int C, int NS>
__device__ __forceinline__ void view_pixel_aa(const T* __restrict__ img, const Rot& R, int H, int W, int h, int w, float tx, float ty,
                                              int i, int j, T* __restrict__ o) {
    float acc[C];
#pragma unroll
    for (int b = 0; b < NS; ++b) {
#pragma unroll
        for (int a = 0; a < NS; ++a) {
            float sx, sy, s[C];
            view_pos(R, H, W, NS * h, NS * w, tx, ty, NS * i + a, NS * j + b, sx, sy);
            sphere_sample_f32<T, C>(img, H, W, sx, sy, s);
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] = a + b == 0 ? s[c] : acc[c] + s[c];
        }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) store_px(o + c, acc[c] / (float)(NS * NS));
}

// view_pixel_aa for a factor known at run time (K20b's tiles); 1 is K12a's pixel itself
template <typename T, int C>
__device__ __forceinline__ void view_pixel_ss(const T* __restrict__ img, const Rot& R, int H, int W, int h, int w, float tx, float ty,
                                              int i, int j, int ss, T* __restrict__ o) {
    switch (ss) {
        case 2: view_pixel_aa<T, C, 2>(img, R, H, W, h, w, tx, ty, i, j, o); break;
        case 3: view_pixel_aa<T, C, 3>(img, R, H, W, h, w, tx, ty, i, j, o); break;
        case 4: view_pixel_aa<T, C, 4>(img, R, H, W, h, w, tx, ty, i, j, o); break;
        default: view_pixel<T, C>(img, R, H, W, h, w, tx, ty, i, j, o); break;
    }
}

// The factor of a frame, as sphere.h's lens a value the kernel asks for.  FactorFixed<NS> is one factor for every frame, known
// when the kernel is compiled: 1 is K12a's pixel, 2 .. 4 K21's.  FactorTable is K22a's factor per frame, int32 [N] on the device:
// uniform over the workgroup, so view_pixel_ss's switch does not diverge; a factor outside 2 .. 4 is 1 there.
template <int NS>
struct FactorFixed {
    template <typename T, int C>
    __device__ __forceinline__ void pixel(const T* __restrict__ img, const Rot& R, int H, int W, int h, int w, float tx, float ty, int i,
                                          int j, int, T* __restrict__ o) const {
        if constexpr (NS == 1) view_pixel<T, C>(img, R, H, W, h, w, tx, ty, i, j, o);
        else view_pixel_aa<T, C, NS>(img, R, H, W, h, w, tx, ty, i, j, o);
    }
};

struct FactorTable {
    const int* ss;
    template <typename T, int C>
    __device__ __forceinline__ void pixel(const T* __restrict__ img, const Rot& R, int H, int W, int h, int w, float tx, float ty, int i,
                                          int j, int frame, T* __restrict__ o) const {
        view_pixel_ss<T, C>(img, R, H, W, h, w, tx, ty, i, j, ss[frame], o);
    }
};

// K12a, K21 and K22a: the view of frame blockIdx.z under its camera, with the (tx, ty) of its lens and its factor.  grid
// (ceil(w / 256), h, N): one thread per view pixel, all C channels, the samples of a factor above 1 one after the other in
// registers.  A tangent that is not finite or not positive decides no address: it ends in the sampler's guard, as a non-finite R.
template <typename T, int C, typename Lens, typename Factor>
__global__ __launch_bounds__(256) void view_render_kernel(const T* __restrict__ src, const float* __restrict__ Rs, const Lens lens,
                                                          const Factor factor, T* __restrict__ dst, int H, int W, int h, int w) {
    const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y, n = blockIdx.z;
    if (i >= w) return;
    const float4 L = lens.at(n);
    const Rot R = load_rot(Rs + (size_t)n * 9);
    factor.template pixel<T, C>(src + (size_t)n * H * W * C, R, H, W, h, w, L.x, L.y, i, j, n, dst + (((size_t)n * h + j) * w + i) * C);
}

// ------------------------------------------------------------------ K20b: several views on one canvas
// The tiles of a canvas, by value: rectangle k = (x0, y0, w, h) shows the view (h, w, tx, ty) of camera k, supersampled ss times
// (K21; 1 = K12a's pixel).  The host has checked that the K <= 8 rectangles are not empty, lie on the canvas and do not overlap
// and that every ss is 1 .. 4.  fill: what a pixel in no tile takes.
constexpr int kMaxTiles = 8;

template <typename T>
struct ViewTiles {
    int x0[kMaxTiles], y0[kMaxTiles], w[kMaxTiles], h[kMaxTiles];
    float tx[kMaxTiles], ty[kMaxTiles];
    int ss[kMaxTiles];
    T fill[4];
    int K;
};

// grid (ceil(wc / 256), hc, N): one thread per canvas pixel.  The scan over the tiles is unrolled: every index into the table is
// a constant, the table stays in the kernel's arguments and the chosen tile in registers.  A pixel in no tile, or in the tile of
// a camera with a non-finite entry, takes fill.  AA = false never reads ss: K20b's kernel as it was, which a canvas whose tiles
// all have the factor 1 takes.
template <typename T, int C, bool AA>
__global__ __launch_bounds__(256) void view_render_multi_kernel(const T* __restrict__ src, const float* __restrict__ Rs,
                                                                T* __restrict__ dst, int H, int W, int hc, int wc,
                                                                const ViewTiles<T> tiles) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= wc) return;
    int sel = -1, i = 0, j = 0, w = 1, h = 1, ss = 1;
    float tx = 0.f, ty = 0.f;
#pragma unroll
    for (int k = 0; k < kMaxTiles; ++k) {
        const int di = x - tiles.x0[k], dj = y - tiles.y0[k];
        if (k < tiles.K && di >= 0 && di < tiles.w[k] && dj >= 0 && dj < tiles.h[k]) {
            sel = k;
            i = di;
            j = dj;
            w = tiles.w[k];
            h = tiles.h[k];
            tx = tiles.tx[k];
            ty = tiles.ty[k];
            if (AA) ss = tiles.ss[k];
        }
    }
    T* o = dst + (((size_t)blockIdx.z * hc + y) * wc + x) * C;
    if (sel >= 0) {
        const Rot R = load_rot(Rs + ((size_t)blockIdx.z * tiles.K + sel) * 9);
        if (rot_finite(R)) {
            if (AA) view_pixel_ss<T, C>(src + (size_t)blockIdx.z * H * W * C, R, H, W, h, w, tx, ty, i, j, ss, o);
            else view_pixel<T, C>(src + (size_t)blockIdx.z * H * W * C, R, H, W, h, w, tx, ty, i, j, o);
            return;
        }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = tiles.fill[c];
}

// ------------------------------------------------------------------ K20a: the caps of earlier cameras taken out of a map
// grid (ceil(P / 256), F): one thread per pixel.  dirs f32 [F][Kx][3]; the pixel is +0 where ((p_x d_x + p_y d_y) + p_z d_z) >= c
// for any k, else the input's bits.  A direction with a non-finite component excludes nothing (an infinite dot would pass the
// comparison, so it is tested).  The loop over the directions is unrolled to its bound of 7: registers only.  Element-wise: out
// may be maps.
constexpr int kMaxCaps = 7;

__device__ __forceinline__ bool in_any_cap(const float* __restrict__ d, int Kx, float px, float py, float pz, float c) {
    bool hit = false;
#pragma unroll
    for (int k = 0; k < kMaxCaps; ++k) {
        if (k < Kx) {
            const float dx = d[3 * k], dy = d[3 * k + 1], dz = d[3 * k + 2];
            const float dot = (px * dx + py * dy) + pz * dz;
            hit = hit || (isfinite(fabsf(dx) + fabsf(dy) + fabsf(dz)) && dot >= c);
        }
    }
    return hit;
}

__global__ __launch_bounds__(256) void view_exclude_kernel(const float* maps, const float* __restrict__ dirs,
                                                           const float2* __restrict__ tabx, const float2* __restrict__ taby,
                                                           float* out, int hm, int wm, int Kx, float c) {
    const int P = hm * wm, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= P) return;
    const int y = j / wm, x = j - y * wm;
    float px, py, pz;
    stab_dir(tabx[x], taby[y], px, py, pz);
    const size_t o = (size_t)blockIdx.y * P + j;
    if (in_any_cap(dirs + (size_t)blockIdx.y * Kx * 3, Kx, px, py, pz, c)) out[o] = 0.f;
    else if (out != maps) out[o] = maps[o];
}

// ------------------------------------------------------------------ K12b, K22b: the view's frame on the panorama
// grid (ceil(W / 256), H, N); element-wise, so dst may be src.  Frame blockIdx.z takes (tx, ty, b) from its lens and compares
// sphere.h's view-frame terms with them.  A frame whose b is not greater than 0 (a NaN too) draws nothing: a table may hold
// one; for the one lens of cp360_view_outline, finite and not below 0, the term changes nothing, since with b = 0 inner is the
// au / av half of inside.
template <typename Lens>
__global__ __launch_bounds__(256) void view_outline_kernel(const uint8_t* src, const float* __restrict__ Rs, const Lens lens,
                                                           const float2* __restrict__ tabx, const float2* __restrict__ taby,
                                                           uint8_t* dst, int H, int W, int cr, int cg, int cb) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const float4 L = lens.at(blockIdx.z);
    const float tx = L.x, ty = L.y, b = L.z;
    const Rot R = load_rot(Rs + (size_t)blockIdx.z * 9);
    float px, py, pz, df, au, av;
    stab_dir(tabx[x], taby[y], px, py, pz);
    view_terms(R, px, py, pz, df, au, av);
    const bool inside = df > 0.f && au <= tx && av <= ty;
    const bool inner = au <= tx - b && av <= ty - b;
    const size_t o = (((size_t)blockIdx.z * H + y) * W + x) * 3;
    if (inside && !inner && b > 0.f && rot_finite(R)) {
        dst[o] = (uint8_t)cr;
        dst[o + 1] = (uint8_t)cg;
        dst[o + 2] = (uint8_t)cb;
    } else if (dst != src) {
        const uint8_t v0 = src[o], v1 = src[o + 1], v2 = src[o + 2];
        dst[o] = v0;
        dst[o + 1] = v1;
        dst[o + 2] = v2;
    }
}

// ------------------------------------------------------------------ K12c: von Mises-Fisher smoothing, all pairs
// grid (ceil(P / 256), F): a workgroup owns 256 output pixels of one frame and walks the frame in LDS tiles of 256 sources
__global__ __launch_bounds__(256) void view_smooth_kernel(const float* __restrict__ maps, const float2* __restrict__ tabx,
                                                          const float2* __restrict__ taby, float* __restrict__ out, int hm, int wm,
                                                          float kappa) {
    __shared__ float4 tile_p[256];                                      // p_j and a_j
    __shared__ float tile_as[256];                                      // a_j s_j
    const int P = hm * wm, tid = threadIdx.x;
    const int i = blockIdx.x * 256 + tid;
    const float* s = maps + (size_t)blockIdx.y * P;
    float pix_x = 1.f, pix_y = 0.f, pix_z = 0.f;
    if (i < P) {
        const int y = i / wm, x = i - y * wm;
        stab_dir(tabx[x], taby[y], pix_x, pix_y, pix_z);
    }
    double num = 0.0, den = 0.0;
    for (int t0 = 0; t0 < P; t0 += 256) {
        const int j = t0 + tid;
        if (j < P) {
            const int y = j / wm, x = j - y * wm;
            const float2 csp = taby[y];
            float qx, qy, qz;
            stab_dir(tabx[x], csp, qx, qy, qz);
            const float sj = s[j];
            tile_p[tid] = make_float4(qx, qy, qz, csp.x);
            tile_as[tid] = csp.x * (isfinite(sj) ? sj : 0.f);
        }
        __syncthreads();
        const int n = P - t0 < 256 ? P - t0 : 256;
        for (int k = 0; k < n; ++k) {
            const float4 q = tile_p[k];
            const float e = vmf(kappa, pix_x, pix_y, pix_z, q.x, q.y, q.z);
            num += (double)(tile_as[k] * e);
            den += (double)(q.w * e);
        }
        __syncthreads();
    }
    if (i < P) out[(size_t)blockIdx.y * P + i] = (float)(num / den);
}

// K12d's mean-shift step, which K16c repeats for given indices: c = sum_j a_j s_j e(p*, p_j) p_j about p* = dir(bi) on the raw map
// s, dir = c / |c| (p* when |c| is 0 or not finite), written by thread 0.  256 threads, all of which call it; thread t takes
// pixels t, t + 256, .. in order, then sphere.h's ordered sum.  red_c is the caller's LDS.
__device__ __forceinline__ void mean_shift_step(const float* __restrict__ s, const float2* __restrict__ tabx,
                                                const float2* __restrict__ taby, int hm, int wm, float kappa, int bi,
                                                double (*red_c)[3], float* __restrict__ dir) {
    const int P = hm * wm, tid = threadIdx.x;
    float cx, cy, cz;
    {
        const int y = bi / wm, x = bi - y * wm;
        stab_dir(tabx[x], taby[y], cx, cy, cz);
    }
    double acc[3] = {0.0, 0.0, 0.0};
    for (int j = tid; j < P; j += 256) {
        const int y = j / wm, x = j - y * wm;
        const float2 csp = taby[y];
        float qx, qy, qz;
        stab_dir(tabx[x], csp, qx, qy, qz);
        const float sj = s[j];
        const float e = vmf(kappa, cx, cy, cz, qx, qy, qz);
        const float wgt = (csp.x * (isfinite(sj) ? sj : 0.f)) * e;
        acc[0] += (double)(wgt * qx);
        acc[1] += (double)(wgt * qy);
        acc[2] += (double)(wgt * qz);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) acc[k] = wave_sum_down(acc[k]);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) red_c[tid >> 6][k] = acc[k];
    }
    __syncthreads();
    if (tid != 0) return;
    const double sx = waves4_sum(&red_c[0][0], 3), sy = waves4_sum(&red_c[0][1], 3), sz = waves4_sum(&red_c[0][2], 3);
    const double n = sqrt(sx * sx + sy * sy + sz * sz);
    float ox = cx, oy = cy, oz = cz;
    if (n > 0.0 && isfinite(n)) {
        ox = (float)(sx / n);
        oy = (float)(sy / n);
        oz = (float)(sz / n);
    }
    dir[0] = ox;
    dir[1] = oy;
    dir[2] = oz;
}

// "look ahead": the direction of a frame without a target, the panorama's centre
__device__ __forceinline__ void look_ahead(float* __restrict__ dir) {
    dir[0] = 1.f;
    dir[1] = 0.f;
    dir[2] = 0.f;
}

// ------------------------------------------------------------------ K12d: the peak and one mean-shift step
// grid F, 256 threads: thread t takes pixels t, t + 256, .. in order, then the shuffle tree, then the 4 waves in order
__global__ __launch_bounds__(256) void view_peak_kernel(const float* __restrict__ smooth, const float* __restrict__ maps,
                                                        const float2* __restrict__ tabx, const float2* __restrict__ taby,
                                                        float* __restrict__ dir_out, int* __restrict__ idx_out,
                                                        float* __restrict__ val_out, int hm, int wm, float kappa) {
    __shared__ float red_v[4];
    __shared__ int red_i[4];
    __shared__ int red_n[4];
    __shared__ double red_c[4][3];
    const int P = hm * wm, tid = threadIdx.x, f = blockIdx.x;
    const float* sm = smooth + (size_t)f * P;
    const float* s = maps + (size_t)f * P;
    // the argmax of the finite smoothed values, lowest index on ties; the number of finite raw values
    float best = 0.f;
    int bi = -1, nfin = 0;
    for (int j = tid; j < P; j += 256) {
        const float v = sm[j];
        if (isfinite(v) && (bi < 0 || v > best)) {
            best = v;
            bi = j;
        }
        nfin += isfinite(s[j]) ? 1 : 0;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) peak_take(__shfl_down(best, off, 64), __shfl_down(bi, off, 64), best, bi);
    nfin = wave_sum_down(nfin);
    if ((tid & 63) == 0) {
        red_v[tid >> 6] = best;
        red_i[tid >> 6] = bi;
        red_n[tid >> 6] = nfin;
    }
    __syncthreads();
    best = red_v[0];
    bi = red_i[0];
#pragma unroll
    for (int k = 1; k < 4; ++k) peak_take(red_v[k], red_i[k], best, bi);
    nfin = waves4_sum(red_n, 1);
    if (bi < 0 || nfin == 0) {                                          // nothing finite: look ahead
        if (tid == 0) {
            look_ahead(dir_out + (size_t)f * 3);
            idx_out[f] = -1;
            val_out[f] = nanf("");
        }
        return;
    }
    mean_shift_step(s, tabx, taby, hm, wm, kappa, bi, red_c, dir_out + (size_t)f * 3);
    if (tid == 0) {
        idx_out[f] = bi;
        val_out[f] = best;
    }
}

// ------------------------------------------------------------------ K22d: how wide the target is
// The larger of two candidates of the cap's peak; have = 0 is no candidate.  A maximum: the order of the visit is free.
__device__ __forceinline__ void spread_take(float ov, int oh, float& top, int& have) {
    if (oh && (!have || ov > top)) {
        top = ov;
        have = 1;
    }
}

// grid F, 256 threads: thread t takes pixels t, t + 256, .. in order, twice.  d = dirs[f]; a pixel is in the cap where
// ((p_x d_x + p_y d_y) + p_z d_z) >= cw.  Pass 1: top = the largest finite s_j in the cap, through the shuffle tree and the four
// waves.  Pass 2: m_j = a_j fmaxf(s_j - lv top, 0) for the finite s_j in the cap, g_j = ((p_x - d_x)^2 + (p_y - d_y)^2 + (p_z -
// d_z)^2) / 2 = 1 - cos of the angle without the cancellation; M = sum m_j and Q = sum m_j g_j in f64 by sphere.h's ordered sum;
// q = (float)(Q / M).  NaN for a non-finite d, a cap without a finite pixel, top <= 0 or an M that is not positive and finite.
// Every exit before a barrier is the whole workgroup's: d, have and top are uniform.
__global__ __launch_bounds__(256) void view_spread_kernel(const float* __restrict__ maps, const float* __restrict__ dirs,
                                                          const float2* __restrict__ tabx, const float2* __restrict__ taby,
                                                          float* __restrict__ q_out, int hm, int wm, float cw, float lv) {
    __shared__ float red_t[4];
    __shared__ int red_h[4];
    __shared__ double red_s[4][2];
    const int P = hm * wm, tid = threadIdx.x, f = blockIdx.x;
    const float* s = maps + (size_t)f * P;
    const float dx = dirs[(size_t)f * 3], dy = dirs[(size_t)f * 3 + 1], dz = dirs[(size_t)f * 3 + 2];
    if (!isfinite(fabsf(dx) + fabsf(dy) + fabsf(dz))) {                 // an infinite dot would pass the comparison
        if (tid == 0) q_out[f] = nanf("");
        return;
    }
    float top = 0.f;
    int have = 0;
    for (int j = tid; j < P; j += 256) {
        const int y = j / wm, x = j - y * wm;
        float px, py, pz;
        stab_dir(tabx[x], taby[y], px, py, pz);
        const float dot = (px * dx + py * dy) + pz * dz;
        const float sj = s[j];
        spread_take(sj, dot >= cw && isfinite(sj), top, have);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) spread_take(__shfl_down(top, off, 64), __shfl_down(have, off, 64), top, have);
    if ((tid & 63) == 0) {
        red_t[tid >> 6] = top;
        red_h[tid >> 6] = have;
    }
    __syncthreads();
    top = red_t[0];
    have = red_h[0];
#pragma unroll
    for (int k = 1; k < 4; ++k) spread_take(red_t[k], red_h[k], top, have);
    if (!have || !(top > 0.f)) {
        if (tid == 0) q_out[f] = nanf("");
        return;
    }
    const float floor_ = lv * top;
    double M = 0.0, Q = 0.0;
    for (int j = tid; j < P; j += 256) {
        const int y = j / wm, x = j - y * wm;
        const float2 csp = taby[y];
        float px, py, pz;
        stab_dir(tabx[x], csp, px, py, pz);
        const float dot = (px * dx + py * dy) + pz * dz;
        const float sj = s[j];
        const float m = dot >= cw && isfinite(sj) ? csp.x * fmaxf(sj - floor_, 0.f) : 0.f;
        const float ex = px - dx, ey = py - dy, ez = pz - dz;
        const float g = 0.5f * ((ex * ex + ey * ey) + ez * ez);
        M += (double)m;
        Q += (double)(m * g);
    }
    M = wave_sum_down(M);
    Q = wave_sum_down(Q);
    if ((tid & 63) == 0) {
        red_s[tid >> 6][0] = M;
        red_s[tid >> 6][1] = Q;
    }
    __syncthreads();
    if (tid != 0) return;
    const double Ms = waves4_sum(&red_s[0][0], 2), Qs = waves4_sum(&red_s[0][1], 2);
    q_out[f] = Ms > 0.0 && isfinite(Ms) ? (float)(Qs / Ms) : nanf("");
}

// ------------------------------------------------------------------ K16: the camera path by dynamic programming
// The table (cp360_path_table_host): cost int32 [hm][hm][wm / 2 + 1] by (row of i, row of j, column difference folded to
// 0 .. wm / 2), -1 = forbidden; behind it span int32 [hm][hm], the largest allowed column difference of the row pair, -1 = none.
constexpr int kPathVoteMax = 4096;
constexpr int kPathThreads = 1024;
constexpr int kPathNone = -(1 << 30);        // below every acc - cost: acc >= 0, cost <= 4096 * 180

__device__ __forceinline__ int path_vote(float s, float g) {
    const float p = s * g;
    return isfinite(p) ? (int)rintf(fminf(fmaxf(p, 0.f), (float)kPathVoteMax)) : 0;
}

__device__ __forceinline__ int path_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// K16a.  grid S, blockDim.x <= 1024 threads and 2 P ints of dynamic LDS: one workgroup walks one sequence, thread k owns the
// states k, k + blockDim.x, ..; the previous and the current frame's scores alternate between the two halves of the LDS, one
// barrier per frame, which every thread reaches: lo and hi are the workgroup's, and no thread leaves early.  A predecessor
// replaces the best so far when acc - cost is larger, or equal at a lower index: the order of the visit does not matter.  The
// table's contents decide no address beyond their own range: spans are clamped to wm / 2, a cost below 0 is skipped, and a state
// that finds no predecessor keeps itself.  The tail is K16b's argmax of the last frame: idx[hi - 1] and score[s].
__global__ __launch_bounds__(kPathThreads) void path_dp_kernel(const float* __restrict__ smooth, const float* __restrict__ gain,
                                                               const int* __restrict__ table, const int* __restrict__ starts,
                                                               uint16_t* __restrict__ back, int* __restrict__ idx_out,
                                                               int* __restrict__ score_out, int F, int hm, int wm) {
    extern __shared__ int path_acc[];                                   // [2][P]
    __shared__ int red_v[kPathThreads / 64];
    __shared__ int red_i[kPathThreads / 64];
    const int P = hm * wm, tid = threadIdx.x, nt = blockDim.x, half = wm / 2 + 1;
    const int* span = table + (size_t)hm * hm * half;
    const int lo = path_clamp(starts[blockIdx.x], 0, F), hi = path_clamp(starts[blockIdx.x + 1], 0, F);
    int* prev = path_acc;
    int* cur = path_acc + P;
    for (int t = lo; t < hi; ++t) {
        const float* s = smooth + (size_t)t * P;
        uint16_t* bk = back + (size_t)t * P;
        const float g = gain[t];
        for (int j = tid; j < P; j += nt) {
            const int q = path_vote(s[j], g);
            const int rj = j / wm, cj = j - rj * wm;
            int best = kPathNone, bi = j;
            if (t == lo) best = 0;
            else {
                // the allowed rows are one interval about rj (the angle grows with the rows' distance): find its first row
                int r0 = rj;
                while (r0 > 0 && span[(r0 - 1) * hm + rj] >= 0) --r0;
                int Dn = span[r0 * hm + rj];
                for (int ri = r0; ri < hm; ++ri) {
                    int D = Dn;
                    Dn = ri + 1 < hm ? span[(ri + 1) * hm + rj] : -1;    // the next row's, in flight behind this row's columns
                    if (D < 0) {
                        if (ri > rj) break;
                        continue;
                    }
                    D = D > wm / 2 ? wm / 2 : D;
                    const bool all = 2 * D + 1 >= wm;                   // every column once: the pole rows
                    const int n = all ? wm : 2 * D + 1;
                    int c = all ? 0 : (cj - D < 0 ? cj - D + wm : cj - D);
                    const int* cost = table + ((size_t)ri * hm + rj) * half;
                    const int* row = prev + ri * wm;
#pragma unroll 4
                    for (int k = 0; k < n; ++k) {
                        int d = c > cj ? c - cj : cj - c;
                        d = d > wm - d ? wm - d : d;
                        const int cst = cost[d], i = ri * wm + c;
                        const int v = row[c] - cst;
                        if (cst >= 0 && (v > best || (v == best && i < bi))) {
                            best = v;
                            bi = i;
                        }
                        c = c + 1 == wm ? 0 : c + 1;
                    }
                }
                if (best == kPathNone) best = 0;                        // a table without the state itself: keep it
            }
            cur[j] = q + best;
            bk[j] = (uint16_t)bi;
        }
        __syncthreads();
        int* const swap = prev;
        prev = cur;
        cur = swap;
    }
    if (lo >= hi) return;                                               // the whole workgroup: lo and hi are uniform
    // prev holds the last frame's scores: their argmax, lowest index on ties
    int best = 0, bi = -1;
    for (int j = tid; j < P; j += nt) {
        const int v = prev[j];
        if (bi < 0 || v > best) {
            best = v;
            bi = j;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) peak_take(__shfl_down(best, off, 64), __shfl_down(bi, off, 64), best, bi);
    if ((tid & 63) == 0) {
        red_v[tid >> 6] = best;
        red_i[tid >> 6] = bi;
    }
    __syncthreads();
    if (tid != 0) return;
    for (int k = 1; k < nt / 64; ++k) peak_take(red_v[k], red_i[k], best, bi);
    idx_out[hi - 1] = bi;
    score_out[blockIdx.x] = best;
}

// K16b.  One thread per sequence, behind K16a on the stream: from idx[hi - 1] back along the back-pointers, hi - lo dependent
// loads; dir = the pixel centre.
__global__ __launch_bounds__(64) void path_trace_kernel(const uint16_t* __restrict__ back, const int* __restrict__ starts,
                                                        const float2* __restrict__ tabx, const float2* __restrict__ taby,
                                                        int* __restrict__ idx_out, float* __restrict__ dir_out, int S, int F,
                                                        int hm, int wm) {
    const int q = blockIdx.x * 64 + threadIdx.x;
    if (q >= S) return;
    const int P = hm * wm;
    const int lo = path_clamp(starts[q], 0, F), hi = path_clamp(starts[q + 1], 0, F);
    if (lo >= hi) return;
    int i = path_clamp(idx_out[hi - 1], 0, P - 1);
    for (int t = hi - 1; t >= lo; --t) {
        const int y = i / wm, x = i - y * wm;
        float px, py, pz;
        stab_dir(tabx[x], taby[y], px, py, pz);
        idx_out[t] = i;
        dir_out[(size_t)t * 3] = px;
        dir_out[(size_t)t * 3 + 1] = py;
        dir_out[(size_t)t * 3 + 2] = pz;
        i = path_clamp((int)back[(size_t)t * P + i], 0, P - 1);
    }
}

// K16c.  grid F, 256 threads: K12d's step about dir(idx[f]); an index outside the map looks ahead
__global__ __launch_bounds__(256) void view_refine_kernel(const float* __restrict__ maps, const int* __restrict__ idx,
                                                          const float2* __restrict__ tabx, const float2* __restrict__ taby,
                                                          float* __restrict__ dir_out, int hm, int wm, float kappa) {
    __shared__ double red_c[4][3];
    const int P = hm * wm, f = blockIdx.x, bi = idx[f];
    if (bi < 0 || bi >= P) {
        if (threadIdx.x == 0) look_ahead(dir_out + (size_t)f * 3);
        return;
    }
    mean_shift_step(maps + (size_t)f * P, tabx, taby, hm, wm, kappa, bi, red_c, dir_out + (size_t)f * 3);
}

// ------------------------------------------------------------------ host side
const double kPi = 3.14159265358979323846;

bool bad_hfov(double hfov) { return !(hfov > 0.0 && hfov < kPi); }

// The lens of a view (h, w) of hfov radians with a border of border_px view pixels, each value rounded to f32 once: what every
// entry point hands its kernel, and a row of cp360_view_lens_host's table (K22)
LensFixed view_lens(double hfov_rad, int h, int w, double border_px) {
    const double t = tan(0.5 * hfov_rad);
    return {(float)t, (float)(t * (double)h / (double)w), border_px == 0.0 ? 0.f : (float)(border_px * 2.0 * t / (double)w)};
}
bool bad_sigma(double sigma) { return !(sigma > 0.0) || !isfinite(sigma); }

template <typename T, int C, typename Lens, typename Factor>
int launch_render(const void* frames, const float* R, Lens lens, Factor factor, void* out, int N, int H, int W, int h, int w,
                  hipStream_t s) {
    hipLaunchKernelGGL((view_render_kernel<T, C, Lens, Factor>), dim3((w + 255) / 256, h, N), dim3(256), 0, s, (const T*)frames, R,
                       lens, factor, (T*)out, H, W, h, w);
    CP360_CHECK_HIP();
    return CP360_OK;
}

// ss = the K factors of K21, or nullptr for K20b as it was (every factor 1)
template <typename T, int C>
int launch_render_multi(const void* frames, const float* R, void* out, int N, int H, int W, int hc, int wc, int K,
                        const int32_t* rects, const float* tx, const float* ty, const int32_t* ss, const void* fill,
                        hipStream_t s) {
    ViewTiles<T> t = {};
    t.K = K;
    for (int k = 0; k < K; ++k) {
        t.x0[k] = rects[4 * k];
        t.y0[k] = rects[4 * k + 1];
        t.w[k] = rects[4 * k + 2];
        t.h[k] = rects[4 * k + 3];
        t.tx[k] = tx[k];
        t.ty[k] = ty[k];
        t.ss[k] = ss ? ss[k] : 1;
    }
    for (int c = 0; c < C; ++c) t.fill[c] = ((const T*)fill)[c];
    const dim3 grid((wc + 255) / 256, hc, N);
    if (ss) hipLaunchKernelGGL((view_render_multi_kernel<T, C, true>), grid, dim3(256), 0, s, (const T*)frames, R, (T*)out, H, W, hc,
                               wc, t);
    else hipLaunchKernelGGL((view_render_multi_kernel<T, C, false>), grid, dim3(256), 0, s, (const T*)frames, R, (T*)out, H, W, hc,
                            wc, t);
    CP360_CHECK_HIP();
    return CP360_OK;
}

// K20b: whether the K rectangles (x0, y0, w, h) are not empty, lie on the hc x wc canvas and share no pixel
bool bad_tiles(const int32_t* rects, int K, int hc, int wc) {
    for (int k = 0; k < K; ++k) {
        const long long x0 = rects[4 * k], y0 = rects[4 * k + 1], w = rects[4 * k + 2], h = rects[4 * k + 3];
        if (w < 1 || h < 1 || x0 < 0 || y0 < 0 || x0 + w > wc || y0 + h > hc) return true;
        for (int m = 0; m < k; ++m) {
            const long long mx = rects[4 * m], my = rects[4 * m + 1], mw = rects[4 * m + 2], mh = rects[4 * m + 3];
            if (x0 < mx + mw && mx < x0 + w && y0 < my + mh && my < y0 + h) return true;
        }
    }
    return false;
}

// the checks smooth and peak share; *kappa = 1 / sigma^2 rounded once
int map_args(int F, int hm, int wm, double sigma_rad, const void* work, size_t work_bytes, float* kappa) {
    if (bad_image(F, hm, wm) || bad_sigma(sigma_rad)) return CP360_ERR_BAD_SHAPE;
    if ((long long)hm * wm > kMaxMapPx || F > 65535) return CP360_ERR_UNSUPPORTED;
    *kappa = (float)(1.0 / (sigma_rad * sigma_rad));
    return check_work(work, work_bytes, tab_bytes(hm, wm));
}

// K16: the shapes of a table / a path; F = 1 stands in where there are no frames
int path_args(int F, int hm, int wm) {
    if (bad_image(F, hm, wm)) return CP360_ERR_BAD_SHAPE;
    return (long long)hm * wm > kMaxMapPx || F > 65535 ? CP360_ERR_UNSUPPORTED : CP360_OK;
}

size_t path_table_ints(int hm, int wm) { return (size_t)hm * hm * (wm / 2 + 1) + (size_t)hm * hm; }
size_t path_back_bytes(int F, int hm, int wm) { return align16((size_t)F * hm * wm * sizeof(uint16_t)); }

// the angle between the pixel centres of rows ri and rj, d columns apart, in radians: atan2(|p x q|, p . q) in double
double path_angle(int hm, int wm, int ri, int rj, int d) {
    const double pi_ = kPi * 0.5 * (1.0 - (2.0 * (double)ri + 1.0) / (double)hm);
    const double pj_ = kPi * 0.5 * (1.0 - (2.0 * (double)rj + 1.0) / (double)hm);
    const double dt = 2.0 * kPi * (double)d / (double)wm;
    const double px = cos(pi_), py = sin(pi_);                          // p at theta 0: pz = 0
    const double qx = cos(pj_) * cos(dt), qy = sin(pj_), qz = cos(pj_) * sin(dt);
    const double cx = py * qz, cy = -px * qz, cz = px * qy - py * qx;
    return atan2(sqrt(cx * cx + cy * cy + cz * cz), px * qx + py * qy);
}

// K16a's 2 P ints of LDS pass the 64 KB a kernel gets unasked: raise the limit once per device, as cubepad.hip does
int path_big_lds() {
    static std::atomic<unsigned long long> done{0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return CP360_ERR_HIP;
    const unsigned long long bit = 1ull << (dev & 63);
    if (!(done.load(std::memory_order_acquire) & bit)) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(path_dp_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                2 * kMaxMapPx * (int)sizeof(int)) != hipSuccess)
            return CP360_ERR_HIP;
        done.fetch_or(bit, std::memory_order_release);
    }
    return CP360_OK;
}

// The checks of every view render, in the order of their statuses.  ss_max is the largest factor a frame may take: the fine view
// (ss h, ss w) must be a view K12a would take, so that the identity with it holds wherever the call is accepted (h, w are
// within big_image's range before they are multiplied).  lens_st is what the entry point found about its own lens and factors:
// CP360_OK, or the status to return where the shared checks reach it.
int render_args(int dtype, const void* frames, const float* R, const void* out, int N, int H, int W, int C, int h, int w, int ss_max,
                int lens_st) {
    if (!frames || !R || !out || lens_st == CP360_ERR_NULL) return CP360_ERR_NULL;
    if (bad_image(N, H, W) || bad_image(N, h, w) || C < 1 || lens_st == CP360_ERR_BAD_SHAPE) return CP360_ERR_BAD_SHAPE;
    if (dtype != CP360_F32 && dtype != CP360_U8) return CP360_ERR_BAD_DTYPE;
    if (C > 4 || (dtype == CP360_U8 && C != 3) || big_image(N, H, W) || big_image(N, h, w) || big_image(N, ss_max * h, ss_max * w))
        return CP360_ERR_UNSUPPORTED;
    if (frames == out) return CP360_ERR_UNSUPPORTED;                   // a gather: not in place
    return lens_st;
}

// K12a and K21: ss = 1 is K12a's pixel
int view_render_ss(int dtype, const void* frames, const float* R, int N, int H, int W, int C, double hfov_rad, int ss, void* out,
                   int h, int w, void* stream) {
    const bool bad = bad_hfov(hfov_rad) || ss < 1 || ss > 4;
    const int st = render_args(dtype, frames, R, out, N, H, W, C, h, w, bad ? 1 : ss, bad ? CP360_ERR_BAD_SHAPE : CP360_OK);
    if (st != CP360_OK) return st;
    const LensFixed lens = view_lens(hfov_rad, h, w, 0.0);
    hipStream_t s = (hipStream_t)stream;
    return dispatch_pixels(dtype, C, [&](auto px, auto c) {
        using T = decltype(px);
        constexpr int Cn = decltype(c)::value;
        switch (ss) {
            case 2: return launch_render<T, Cn>(frames, R, lens, FactorFixed<2>(), out, N, H, W, h, w, s);
            case 3: return launch_render<T, Cn>(frames, R, lens, FactorFixed<3>(), out, N, H, W, h, w, s);
            case 4: return launch_render<T, Cn>(frames, R, lens, FactorFixed<4>(), out, N, H, W, h, w, s);
            default: return launch_render<T, Cn>(frames, R, lens, FactorFixed<1>(), out, N, H, W, h, w, s);
        }
    });
}

// K12b and K22b: the checks of both entry points, the tables and the launch; lens_st as render_args's
template <typename Lens>
int view_outline(const uint8_t* frames, const float* R, Lens lens, int lens_st, int N, int H, int W, const uint8_t* rgb, uint8_t* out,
                 void* work, size_t work_bytes, void* stream) {
    if (!frames || !R || !rgb || !out || !work || lens_st == CP360_ERR_NULL) return CP360_ERR_NULL;
    if (bad_image(N, H, W) || lens_st == CP360_ERR_BAD_SHAPE) return CP360_ERR_BAD_SHAPE;
    if (big_image(N, H, W)) return CP360_ERR_UNSUPPORTED;
    if (lens_st != CP360_OK) return lens_st;
    hipStream_t s = (hipStream_t)stream;
    SphereTabs tabs;
    const int st = open_tabs(work, work_bytes, tab_bytes(H, W), H, W, s, &tabs);
    if (st != CP360_OK) return st;
    hipLaunchKernelGGL(view_outline_kernel<Lens>, dim3((W + 255) / 256, H, N), dim3(256), 0, s, frames, R, lens, tabs.x, tabs.y, out, H,
                       W, (int)rgb[0], (int)rgb[1], (int)rgb[2]);
    CP360_CHECK_HIP();
    return CP360_OK;
}

}  // namespace

// ------------------------------------------------------------------ C ABI
extern "C" int cp360_view_render(int dtype, const void* frames, const float* R, int N, int H, int W, int C, double hfov_rad,
                                 void* out, int h, int w, void* stream) {
    return view_render_ss(dtype, frames, R, N, H, W, C, hfov_rad, 1, out, h, w, stream);
}

extern "C" int cp360_view_render_aa(int dtype, const void* frames, const float* R, int N, int H, int W, int C, double hfov_rad,
                                    int ss, void* out, int h, int w, void* stream) {
    return view_render_ss(dtype, frames, R, N, H, W, C, hfov_rad, ss, out, h, w, stream);
}

extern "C" int cp360_view_outline(const uint8_t* frames, const float* R, int N, int H, int W, double hfov_rad, int h, int w,
                                  double border_px, const uint8_t* rgb, uint8_t* out, void* work, size_t work_bytes, void* stream) {
    const bool bad = bad_image(N, h, w) || bad_hfov(hfov_rad) || !(border_px > 0.0) || !isfinite(border_px);
    const LensFixed lens = bad ? LensFixed{} : view_lens(hfov_rad, h, w, border_px);
    return view_outline(frames, R, lens, bad ? CP360_ERR_BAD_SHAPE : CP360_OK, N, H, W, rgb, out, work, work_bytes, stream);
}

extern "C" int cp360_view_smooth(const float* maps, int F, int hm, int wm, double sigma_rad, float* out, void* work,
                                 size_t work_bytes, void* stream) {
    if (!maps || !out || !work) return CP360_ERR_NULL;
    float kappa = 0.f;
    int st = map_args(F, hm, wm, sigma_rad, work, work_bytes, &kappa);
    if (st != CP360_OK) return st;
    if (maps == out) return CP360_ERR_UNSUPPORTED;                     // every output reads every input
    hipStream_t s = (hipStream_t)stream;
    SphereTabs t;
    st = launch_tables(work, hm, wm, s, &t);
    if (st != CP360_OK) return st;
    hipLaunchKernelGGL(view_smooth_kernel, dim3((hm * wm + 255) / 256, F), dim3(256), 0, s, maps, t.x, t.y, out, hm, wm, kappa);
    CP360_CHECK_HIP();
    return CP360_OK;
}

extern "C" int cp360_view_peak(const float* smooth, const float* maps, int F, int hm, int wm, double sigma_rad, float* dir_out,
                               int* idx_out, float* val_out, void* work, size_t work_bytes, void* stream) {
    if (!smooth || !maps || !dir_out || !idx_out || !val_out || !work) return CP360_ERR_NULL;
    float kappa = 0.f;
    int st = map_args(F, hm, wm, sigma_rad, work, work_bytes, &kappa);
    if (st != CP360_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    SphereTabs t;
    st = launch_tables(work, hm, wm, s, &t);
    if (st != CP360_OK) return st;
    hipLaunchKernelGGL(view_peak_kernel, dim3(F), dim3(256), 0, s, smooth, maps, t.x, t.y, dir_out, idx_out, val_out, hm, wm, kappa);
    CP360_CHECK_HIP();
    return CP360_OK;
}

// ------------------------------------------------------------------ K16: the camera path
extern "C" size_t cp360_path_table_bytes(int hm, int wm) {
    return path_args(1, hm, wm) != CP360_OK ? 0 : path_table_ints(hm, wm) * sizeof(int32_t);
}

extern "C" int cp360_path_table_host(int hm, int wm, double turn_cost, double step_rad, int32_t* out) {
    if (!out) return CP360_ERR_NULL;
    if (bad_image(1, hm, wm) || !(turn_cost >= 0.0 && turn_cost <= 4096.0) || !(step_rad > 0.0 && step_rad <= kPi))
        return CP360_ERR_BAD_SHAPE;
    const int st = path_args(1, hm, wm);
    if (st != CP360_OK) return st;
    const int half = wm / 2 + 1;
    int32_t* span = out + (size_t)hm * hm * half;
    for (int ri = 0; ri < hm; ++ri) {
        for (int rj = ri; rj < hm; ++rj) {                              // the mirror image is a copy: symmetric to the bit
            int32_t* c = out + ((size_t)ri * hm + rj) * half;
            int D = -1;
            for (int d = 0; d < half; ++d) {
                const double a = path_angle(hm, wm, ri, rj, d);
                const bool ok = D == d - 1 && a <= step_rad;            // one interval: nothing behind the first forbidden one
                c[d] = ok ? (int32_t)rint(turn_cost * (a * (180.0 / kPi))) : -1;
                if (ok) D = d;
            }
            span[ri * hm + rj] = span[rj * hm + ri] = D;
            int32_t* m = out + ((size_t)rj * hm + ri) * half;
            for (int d = 0; d < half && m != c; ++d) m[d] = c[d];
        }
    }
    return CP360_OK;
}

extern "C" size_t cp360_path_work_bytes(int F, int hm, int wm) {
    return path_args(F, hm, wm) != CP360_OK ? 0 : tab_bytes(hm, wm) + path_back_bytes(F, hm, wm);
}

extern "C" int cp360_view_path(const float* smooth, const float* gain, int F, int hm, int wm, const int32_t* table_dev,
                               const int32_t* starts_dev, int S, int32_t* idx_out, float* dir_out, int32_t* score_out, void* work,
                               size_t work_bytes, void* stream) {
    if (!smooth || !gain || !table_dev || !starts_dev || !idx_out || !dir_out || !score_out || !work) return CP360_ERR_NULL;
    if (bad_image(F, hm, wm) || S < 1 || S > F) return CP360_ERR_BAD_SHAPE;
    int st = path_args(F, hm, wm);
    if (st != CP360_OK) return st;
    st = check_work(work, work_bytes, cp360_path_work_bytes(F, hm, wm));
    if (st != CP360_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    SphereTabs t;
    st = launch_tables(work, hm, wm, s, &t);
    if (st != CP360_OK) return st;
    st = path_big_lds();
    if (st != CP360_OK) return st;
    const int P = hm * wm;
    const int threads = P >= kPathThreads ? kPathThreads : (P + 63) / 64 * 64;
    uint16_t* back = (uint16_t*)((char*)work + tab_bytes(hm, wm));
    hipLaunchKernelGGL(path_dp_kernel, dim3(S), dim3(threads), 2 * (size_t)P * sizeof(int), s, smooth, gain, (const int*)table_dev,
                       (const int*)starts_dev, back, (int*)idx_out, (int*)score_out, F, hm, wm);
    CP360_CHECK_HIP();
    hipLaunchKernelGGL(path_trace_kernel, dim3((S + 63) / 64), dim3(64), 0, s, (const uint16_t*)back, (const int*)starts_dev, t.x, t.y,
                       (int*)idx_out, dir_out, S, F, hm, wm);
    CP360_CHECK_HIP();
    return CP360_OK;
}

extern "C" int cp360_view_refine(const float* maps, const int32_t* idx, int F, int hm, int wm, double sigma_rad, float* dir_out,
                                 void* work, size_t work_bytes, void* stream) {
    if (!maps || !idx || !dir_out || !work) return CP360_ERR_NULL;
    float kappa = 0.f;
    int st = map_args(F, hm, wm, sigma_rad, work, work_bytes, &kappa);
    if (st != CP360_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    SphereTabs t;
    st = launch_tables(work, hm, wm, s, &t);
    if (st != CP360_OK) return st;
    hipLaunchKernelGGL(view_refine_kernel, dim3(F), dim3(256), 0, s, maps, (const int*)idx, t.x, t.y, dir_out, hm, wm, kappa);
    CP360_CHECK_HIP();
    return CP360_OK;
}

// ------------------------------------------------------------------ K20: several cameras at once
extern "C" int cp360_view_exclude(const float* maps, const float* dirs, int F, int hm, int wm, int Kx, double radius_rad, float* out,
                                  void* work, size_t work_bytes, void* stream) {
    if (!maps || !dirs || !out || !work) return CP360_ERR_NULL;
    if (bad_image(F, hm, wm) || Kx < 1 || Kx > kMaxCaps || !(radius_rad > 0.0 && radius_rad <= kPi)) return CP360_ERR_BAD_SHAPE;
    int st = path_args(F, hm, wm);
    if (st != CP360_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    SphereTabs t;
    st = open_tabs(work, work_bytes, tab_bytes(hm, wm), hm, wm, s, &t);
    if (st != CP360_OK) return st;
    const float c = (float)cos(radius_rad);
    hipLaunchKernelGGL(view_exclude_kernel, dim3((hm * wm + 255) / 256, F), dim3(256), 0, s, maps, dirs, t.x, t.y, out, hm, wm, Kx, c);
    CP360_CHECK_HIP();
    return CP360_OK;
}

// K20b and K21 behind one list of checks: ss = nullptr is K20b (every factor 1), and so is a list of ones.  A tile lies on the
// canvas, so its (h, w) are within big_image's range before they are multiplied.
static int view_render_multi_ss(int dtype, const void* frames, const float* R, int N, int H, int W, int C, int K,
                                const int32_t* tiles, const double* hfov_rad, const int32_t* ss, const void* fill, void* out, int hc,
                                int wc, void* stream) {
    if (bad_image(N, H, W) || bad_image(N, hc, wc) || C < 1 || K < 1 || K > kMaxTiles) return CP360_ERR_BAD_SHAPE;
    for (int k = 0; k < K; ++k)
        if (bad_hfov(hfov_rad[k])) return CP360_ERR_BAD_SHAPE;
    if (bad_tiles(tiles, K, hc, wc)) return CP360_ERR_BAD_SHAPE;
    bool ones = true;
    for (int k = 0; ss && k < K; ++k) {
        if (ss[k] < 1 || ss[k] > 4) return CP360_ERR_BAD_SHAPE;
        ones = ones && ss[k] == 1;
    }
    if (dtype != CP360_F32 && dtype != CP360_U8) return CP360_ERR_BAD_DTYPE;
    if (C > 4 || (dtype == CP360_U8 && C != 3) || big_image(N, H, W) || big_image(N, hc, wc)) return CP360_ERR_UNSUPPORTED;
    for (int k = 0; ss && k < K; ++k)
        if (big_image(N, ss[k] * tiles[4 * k + 3], ss[k] * tiles[4 * k + 2])) return CP360_ERR_UNSUPPORTED;
    if (frames == out) return CP360_ERR_UNSUPPORTED;                   // a gather: not in place
    float tx[kMaxTiles], ty[kMaxTiles];
    for (int k = 0; k < K; ++k) {                                       // cp360_view_render's, per tile
        const LensFixed lens = view_lens(hfov_rad[k], tiles[4 * k + 3], tiles[4 * k + 2], 0.0);
        tx[k] = lens.tx;
        ty[k] = lens.ty;
    }
    hipStream_t s = (hipStream_t)stream;
    return dispatch_pixels(dtype, C, [&](auto px, auto c) {
        return launch_render_multi<decltype(px), decltype(c)::value>(frames, R, out, N, H, W, hc, wc, K, tiles, tx, ty,
                                                                     ones ? nullptr : ss, fill, s);
    });
}

extern "C" int cp360_view_render_multi(int dtype, const void* frames, const float* R, int N, int H, int W, int C, int K,
                                       const int32_t* tiles, const double* hfov_rad, const void* fill, void* out, int hc, int wc,
                                       void* stream) {
    if (!frames || !R || !tiles || !hfov_rad || !fill || !out) return CP360_ERR_NULL;
    return view_render_multi_ss(dtype, frames, R, N, H, W, C, K, tiles, hfov_rad, nullptr, fill, out, hc, wc, stream);
}

extern "C" int cp360_view_render_multi_aa(int dtype, const void* frames, const float* R, int N, int H, int W, int C, int K,
                                          const int32_t* tiles, const double* hfov_rad, const int32_t* ss, const void* fill,
                                          void* out, int hc, int wc, void* stream) {
    if (!frames || !R || !tiles || !hfov_rad || !ss || !fill || !out) return CP360_ERR_NULL;
    return view_render_multi_ss(dtype, frames, R, N, H, W, C, K, tiles, hfov_rad, ss, fill, out, hc, wc, stream);
}

// ------------------------------------------------------------------ K22: zoom, a lens per frame
extern "C" int cp360_view_lens_host(const double* hfov_rad, int N, int h, int w, double border_px, float* lens) {
    if (!hfov_rad || !lens) return CP360_ERR_NULL;
    if (bad_image(N, h, w) || !(border_px >= 0.0) || !isfinite(border_px)) return CP360_ERR_BAD_SHAPE;
    for (int n = 0; n < N; ++n)
        if (bad_hfov(hfov_rad[n])) return CP360_ERR_BAD_SHAPE;
    for (int n = 0; n < N; ++n) {
        const LensFixed l = view_lens(hfov_rad[n], h, w, border_px);
        lens[4 * n] = l.tx;
        lens[4 * n + 1] = l.ty;
        lens[4 * n + 2] = l.b;
        lens[4 * n + 3] = 0.f;
    }
    return CP360_OK;
}

// view_render_ss with the lens in place of the field of view; the alignment is its last check
extern "C" int cp360_view_render_zoom(int dtype, const void* frames, const float* R, const float* lens, const int32_t* ss, int N,
                                      int H, int W, int C, void* out, int h, int w, void* stream) {
    const int lens_st = !lens ? CP360_ERR_NULL : (!aligned16(lens) || ((uintptr_t)ss & 3) != 0 ? CP360_ERR_ALIGN : CP360_OK);
    const int st = render_args(dtype, frames, R, out, N, H, W, C, h, w, ss ? 4 : 1, lens_st);
    if (st != CP360_OK) return st;
    const LensTable table = {(const float4*)lens};
    hipStream_t s = (hipStream_t)stream;
    return dispatch_pixels(dtype, C, [&](auto px, auto c) {
        using T = decltype(px);
        constexpr int Cn = decltype(c)::value;
        if (ss) return launch_render<T, Cn>(frames, R, table, FactorTable{(const int*)ss}, out, N, H, W, h, w, s);
        return launch_render<T, Cn>(frames, R, table, FactorFixed<1>(), out, N, H, W, h, w, s);
    });
}

extern "C" int cp360_view_outline_zoom(const uint8_t* frames, const float* R, const float* lens, int N, int H, int W,
                                       const uint8_t* rgb, uint8_t* out, void* work, size_t work_bytes, void* stream) {
    const int lens_st = !lens ? CP360_ERR_NULL : (!aligned16(lens) ? CP360_ERR_ALIGN : CP360_OK);
    return view_outline(frames, R, LensTable{(const float4*)lens}, lens_st, N, H, W, rgb, out, work, work_bytes, stream);
}

extern "C" int cp360_view_spread(const float* maps, const float* dirs, int F, int hm, int wm, double window_rad, double level,
                                 float* q, void* work, size_t work_bytes, void* stream) {
    if (!maps || !dirs || !q || !work) return CP360_ERR_NULL;
    if (bad_image(F, hm, wm) || !(window_rad > 0.0 && window_rad <= kPi) || !(level > 0.0 && level < 1.0))
        return CP360_ERR_BAD_SHAPE;
    int st = path_args(F, hm, wm);
    if (st != CP360_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    SphereTabs t;
    st = open_tabs(work, work_bytes, tab_bytes(hm, wm), hm, wm, s, &t);
    if (st != CP360_OK) return st;
    hipLaunchKernelGGL(view_spread_kernel, dim3(F), dim3(256), 0, s, maps, dirs, t.x, t.y, q, hm, wm, (float)cos(window_rad),
                       (float)level);
    CP360_CHECK_HIP();
    return CP360_OK;
}
