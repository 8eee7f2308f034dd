// K26: the quality of a decoded video against its source, on the sphere and per cell - the weighted squared error behind WS-PSNR
// and a windowed structural similarity on integer luma behind WS-SSIM.  The reference has no counterpart; the specification is
// the package's own, DESIGN.md "K26" (7r), and tests/quality_restate.py restates it in numpy integers.
//
//   ref, dist u8 [F, H, W, 3]; pixel (y, x) lies in cell ((y rows) / H, (x cols) / W) (K24's tile rule); a_y = K13's row weights
//   sse[f, t, c]  = sum over the pixels of cell t of a_y (ref - dist)^2                                     int64 [F, rows cols, 3]
//   Y             = (4899 R + 9617 G + 1868 B + 8192) >> 14 (K10's luma); a 4 x 4 block has s1 = sum Yr, s2 = sum Yd,
//                   ss = sum (Yr^2 + Yd^2), s12 = sum Yr Yd; window (i, j) = the blocks (i, j), (i, j + 1), (i + 1, j), (i + 1, j + 1),
//                   column j + 1 modulo W / 4: 8 x 8 pixels at stride 4, across the seam, never across a pole
//   q             = rint((double)A / (double)B 2^24), A = (2 s1 s2 + 416)(2 covar + 235963), B = (s1^2 + s2^2 + 416)(vars + 235963),
//                   vars = 64 ss - s1^2 - s2^2, covar = 64 s12 - s1 s2 (int64; one f64 quotient per window)
//   ssim_q[f, t]  = sum over the windows whose pixel (4 i + 4, (4 j + 4) % W) lies in cell t of ww_i q, ww_i = a_4i + .. + a_4i+7
// Integers only outside the quotient: no result depends on the order of accumulation, on the launch geometry, on F or on the
// byte address of the frames.
//
// K26b reads every byte once.  A workgroup of 4 waves owns up to 256 blocks of columns (1024 pixels) and a band of block rows of
// one frame pair and walks down the band, four pixel rows of both videos at a time: the eight lines are read in 16-byte vectors
// from the 16-byte boundary below each line's first byte, whatever the two addresses (a vector that is not wholly inside the
// caller's buffer is read byte by byte), one step ahead of their use, and left in LDS as they lie in memory.  A thread then owns
// four columns: it takes its 12 bytes of a line as four aligned LDS words shifted by the line's byte phase, so the squared errors
// and the luma sums come from the same loads.  A thread's columns fix its cells: a_y (r - d)^2 adds up in u32 registers per
// column (one term < 2^26: 32 rows hold), goes to the workgroup's u64 sums of the current cell row in LDS after 32 rows or where
// the cell row ends, and from there to the result with one 64-bit integer atomic per cell and channel: a destination meets one
// adder per band and column chunk that its cell touches (DESIGN 7r counts them: at most 4 on fine cells, 8 on 6 x 12 tiles of
// 64 frames of 2048 x 4096, more where few frames shrink the bands to as little as 16 rows), not one per row.  The block sums of the row of blocks below are the next
// step's: a thread keeps the pair sums of the step before in registers, the column to its right comes through LDS, the one
// beyond the workgroup's last is summed by 16 lanes from 16 pixels read for that purpose, and a band reads the block row below
// its last one again (the halo: 1 / 32 of a frame).  cols close to W (W / cols < 4): 64 blocks of columns per workgroup, so that
// the cells of a workgroup still fit its LDS sums - slower, the same bits.
#include "sphere.h"

namespace {

constexpr int kQThreads = 256;               // threads = blocks of columns of a workgroup at most
constexpr int kQLines = 8;                   // 4 pixel rows of both videos
constexpr int kQVec = 194;                   // 16-byte vectors of a line: 15 + 12 * 256 + 15 bytes at most, rounded up, + 1 for the 4th word
constexpr int kQCells = 258;                 // cell columns a workgroup can meet: 257, and the window column across the seam
constexpr int kQFlushRows = 32;              // rows a u32 column sum holds: 32 * 65025 * 1024 < 2^32
constexpr int kQMaxW = 1 << 21;

struct QGeom {
    int F, H, W, rows, cols;
    int cw, nchunks;                         // blocks of columns per workgroup, workgroups per row
    int band, nbands;                        // block rows per workgroup, workgroups per column
};

// ------------------------------------------------------------------ K26a: the cell of every column and row, the weights
// colcell int32 [W], rowcell int32 [H], aw int32 [H] (a_y clamped to 0 .. 1024), ww int32 [H / 4] (ww_i, 0 where no window)
__global__ __launch_bounds__(256) void quality_tables_kernel(const int* __restrict__ wrow, int* __restrict__ colcell,
                                                             int* __restrict__ rowcell, int* __restrict__ aw, int* __restrict__ ww,
                                                             int H, int W, int rows, int cols) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < W) colcell[i] = (int)(((long long)i * cols) / W);
    if (i < H) {
        rowcell[i] = (int)(((long long)i * rows) / H);
        aw[i] = fix_clamp(wrow[i], 0, 1024);
    }
    if (i < H / 4) {
        int s = 0;
        if (4 * i + 8 <= H)
            for (int r = 0; r < 8; ++r) s += fix_clamp(wrow[4 * i + r], 0, 1024);
        ww[i] = s;
    }
}

// the 16 bytes at p, which may lie partly outside [lo, hi): those bytes are 0
__device__ __forceinline__ uint4 quality_load(const uint8_t* p, const uint8_t* lo, const uint8_t* hi) {
    if (p >= lo && p + 16 <= hi) return *reinterpret_cast<const uint4*>(p);
    unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 16; ++j)
        if (p + j >= lo && p + j < hi) w[j >> 2] |= (unsigned)p[j] << (8 * (j & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// the pixel at p (inside [lo, hi)) as R | G << 8 | B << 16: the two aligned words around it where both lie inside the buffer,
// else its three bytes
__device__ __forceinline__ unsigned quality_pixel(const uint8_t* p, const uint8_t* lo, const uint8_t* hi) {
    const unsigned sh = (unsigned)((uintptr_t)p & 3);
    const uint8_t* a = p - sh;
    if (a >= lo && a + 8 <= hi) {
        const unsigned w0 = reinterpret_cast<const unsigned*>(a)[0], w1 = reinterpret_cast<const unsigned*>(a)[1];
        return (unsigned)((((unsigned long long)w1 << 32) | w0) >> (8u * sh)) & 0xffffffu;
    }
    return (unsigned)p[0] | (unsigned)p[1] << 8 | (unsigned)p[2] << 16;
}

__device__ __forceinline__ unsigned quality_luma(unsigned r, unsigned g, unsigned b) {
    return (4899u * r + 9617u * g + 1868u * b + 8192u) >> 14;
}

// byte j (0 .. 11) of three words
#define QBYTE(w, j) (((w)[(j) >> 2] >> (8 * ((j) & 3))) & 255u)

// ------------------------------------------------------------------ K26b: both sums of a band of one frame pair
// grid (nchunks nbands, F), 256 threads
template <bool SSIM>
__global__ __launch_bounds__(kQThreads) void quality_kernel(const uint8_t* __restrict__ ref, const uint8_t* __restrict__ dist,
                                                            const int* __restrict__ colcell, const int* __restrict__ rowcell,
                                                            const int* __restrict__ aw, const int* __restrict__ ww,
                                                            unsigned long long* __restrict__ sse,
                                                            unsigned long long* __restrict__ ssim, const QGeom g) {
    __shared__ uint4 stage[kQLines * kQVec];
    __shared__ unsigned long long cacc[kQCells * 3];
    __shared__ unsigned long long sacc[kQCells];
    __shared__ uint4 bsum[kQThreads];
    __shared__ unsigned hal[4];

    const int tid = threadIdx.x;
    const int H = g.H, W = g.W, cols = g.cols;
    const int chunk = blockIdx.x % g.nchunks, bandi = blockIdx.x / g.nchunks, f = blockIdx.y;
    const int NB = (W + 3) >> 2, NBR = (H + 3) >> 2;
    const int b0 = chunk * g.cw;
    const int cwa = g.cw < NB - b0 ? g.cw : NB - b0;                    // this workgroup's blocks of columns
    const int r0 = bandi * g.band;
    const int r1 = r0 + g.band < NBR ? r0 + g.band : NBR;
    const int iend = SSIM && r1 < NBR ? r1 : r1 - 1;                    // with the halo block row
    const size_t rb = (size_t)3 * W;
    const size_t xb0 = (size_t)12 * b0;
    const int nbytes = (int)((size_t)12 * cwa < rb - xb0 ? (size_t)12 * cwa : rb - xb0);
    const size_t T = (size_t)g.rows * cols;
    const uint8_t* const lo_r = ref;
    const uint8_t* const hi_r = ref + (size_t)g.F * H * rb;
    const uint8_t* const lo_d = dist;
    const uint8_t* const hi_d = dist + (size_t)g.F * H * rb;

    for (int k = tid; k < kQCells * 3; k += kQThreads) cacc[k] = 0ull;
    for (int k = tid; k < kQCells; k += kQThreads) sacc[k] = 0ull;

    // this thread's columns and their cells, local to the workgroup's first one
    const bool active = tid < cwa;
    const int x0 = 4 * (b0 + tid);
    const int cbase = colcell[4 * b0];
    int lc[4];
    unsigned msk[3] = {0u, 0u, 0u};                                    // the bytes of the thread's 12 that are pixels of the row
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = x0 + k;
        lc[k] = active ? colcell[x < W ? x : W - 1] - cbase : 0;
        if (active && x < W) {
#pragma unroll
            for (int c = 0; c < 3; ++c) msk[(3 * k + c) >> 2] |= 255u << (8 * ((3 * k + c) & 3));
        }
    }
    int wl = 0;                                                        // the cell column of the thread's windows
    if (SSIM && active) {
        wl = colcell[(x0 + 4) % W] - cbase;
        if (wl < 0) wl += cols;
    }
    const int xh = (4 * (b0 + cwa)) % W;                               // the block of columns beyond the workgroup's last

    unsigned P[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k) P[k][0] = P[k][1] = P[k][2] = 0u;
    int nrowsP = 0, cur = -1, scur = -1;
    long long sq = 0;
    unsigned hp1 = 0u, hp2 = 0u, hps = 0u, hp12 = 0u;                  // the pair sums of the block row above

    uint4 pre[kQLines];
    unsigned prh_r = 0u, prh_d = 0u;
    auto load_step = [&](int i) {
#pragma unroll
        for (int l = 0; l < kQLines; ++l) {
            pre[l] = make_uint4(0u, 0u, 0u, 0u);
            const int y = 4 * i + (l & 3);
            if (y < H) {
                const uint8_t* row = (l < 4 ? ref : dist) + ((size_t)f * H + y) * rb + xb0;
                const int d = (int)((uintptr_t)row & 15);
                if (tid < ((d + nbytes + 15) >> 4)) pre[l] = quality_load(row - d + 16 * tid, l < 4 ? lo_r : lo_d, l < 4 ? hi_r : hi_d);
            }
        }
        if (SSIM && tid < 16) {                                        // pixel (tid / 4, tid % 4) of the block beyond the last
            const size_t o = (((size_t)f * H + 4 * i + (tid >> 2)) * W + xh + (tid & 3)) * 3;
            prh_r = quality_pixel(ref + o, lo_r, hi_r);
            prh_d = quality_pixel(dist + o, lo_d, hi_d);
        }
    };

    auto flush_cols = [&]() {                                          // the thread's column sums -> the workgroup's cell sums
        if (active && nrowsP > 0) {
            if (lc[0] == lc[3]) {
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    atomicAdd(&cacc[lc[0] * 3 + c], (unsigned long long)P[0][c] + P[1][c] + P[2][c] + P[3][c]);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int c = 0; c < 3; ++c) atomicAdd(&cacc[lc[k] * 3 + c], (unsigned long long)P[k][c]);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) P[k][0] = P[k][1] = P[k][2] = 0u;
        }
        nrowsP = 0;
    };
    auto flush_cells = [&]() {                                         // the workgroup's cell sums of cell row cur -> the result
        flush_cols();
        __syncthreads();
        if (cur >= 0) {
            for (int k = tid; k < kQCells * 3; k += kQThreads) {
                const unsigned long long v = cacc[k];
                if (v != 0ull) {
                    atomicAdd(&sse[((size_t)f * T + (size_t)cur * cols + cbase + k / 3) * 3 + k % 3], v);
                    cacc[k] = 0ull;
                }
            }
        }
        __syncthreads();
    };
    auto flush_windows = [&]() {                                       // the same for the windows of cell row scur
        if (sq != 0) atomicAdd(&sacc[wl], (unsigned long long)sq);
        sq = 0;
        __syncthreads();
        if (scur >= 0) {
            for (int k = tid; k < kQCells; k += kQThreads) {
                const unsigned long long v = sacc[k];
                if (v != 0ull) {
                    atomicAdd(&ssim[(size_t)f * T + (size_t)scur * cols + (cbase + k) % cols], v);
                    sacc[k] = 0ull;
                }
            }
        }
        __syncthreads();
    };

    load_step(r0);
    for (int i = r0; i <= iend; ++i) {
        __syncthreads();                                               // the step before has read its lines (and the sums are zero)
#pragma unroll
        for (int l = 0; l < kQLines; ++l)
            if (tid < kQVec) stage[l * kQVec + tid] = pre[l];
        const unsigned hr = prh_r, hd = prh_d;
        if (SSIM && tid < 4) hal[tid] = 0u;
        __syncthreads();
        if (i < iend) load_step(i + 1);

        const bool own = i < r1;                                       // not the halo: its squared errors are the next band's
        unsigned s1 = 0u, s2 = 0u, ss = 0u, s12 = 0u;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int y = 4 * i + r;
            if (y >= H) break;
            if (own) {
                const int cr = rowcell[y];
                if (cr != cur) {
                    flush_cells();
                    cur = cr;
                }
            }
            if (active) {
                unsigned a[2][3];
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    const uint8_t* row = (m == 0 ? ref : dist) + ((size_t)f * H + y) * rb + xb0;
                    const unsigned o = (unsigned)((uintptr_t)row & 15) + 12u * (unsigned)tid;
                    const unsigned* w = reinterpret_cast<const unsigned*>(stage + (m * 4 + r) * kQVec) + (o >> 2);
                    const unsigned w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3];
                    const unsigned sh = (o & 3u) * 8u;
                    a[m][0] = (unsigned)((((unsigned long long)w1 << 32) | w0) >> sh) & msk[0];
                    a[m][1] = (unsigned)((((unsigned long long)w2 << 32) | w1) >> sh) & msk[1];
                    a[m][2] = (unsigned)((((unsigned long long)w3 << 32) | w2) >> sh) & msk[2];
                }
                if (own) {
                    const unsigned ay = (unsigned)aw[y];
#pragma unroll
                    for (int k = 0; k < 4; ++k)
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            const int dd = (int)QBYTE(a[0], 3 * k + c) - (int)QBYTE(a[1], 3 * k + c);
                            P[k][c] += __umul24((unsigned)(dd * dd), ay);
                        }
                }
                if (SSIM) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const unsigned yr = quality_luma(QBYTE(a[0], 3 * k), QBYTE(a[0], 3 * k + 1), QBYTE(a[0], 3 * k + 2));
                        const unsigned yd = quality_luma(QBYTE(a[1], 3 * k), QBYTE(a[1], 3 * k + 1), QBYTE(a[1], 3 * k + 2));
                        s1 += yr;
                        s2 += yd;
                        ss += yr * yr + yd * yd;
                        s12 += yr * yd;
                    }
                }
            }
            if (own && ++nrowsP == kQFlushRows) flush_cols();
        }
        if (SSIM) {
            bsum[tid] = make_uint4(s1, s2, ss, s12);
            if (tid < 16) {
                const unsigned yr = quality_luma(hr & 255u, (hr >> 8) & 255u, hr >> 16);
                const unsigned yd = quality_luma(hd & 255u, (hd >> 8) & 255u, hd >> 16);
                atomicAdd(&hal[0], yr);
                atomicAdd(&hal[1], yd);
                atomicAdd(&hal[2], yr * yr + yd * yd);
                atomicAdd(&hal[3], yr * yd);
            }
            __syncthreads();
            if (active) {
                const uint4 nb = tid + 1 < cwa ? bsum[tid + 1] : make_uint4(hal[0], hal[1], hal[2], hal[3]);
                s1 += nb.x;
                s2 += nb.y;
                ss += nb.z;
                s12 += nb.w;
            }
            if (i > r0) {                                              // window row i - 1: the block rows i - 1 and i
                const int wr = rowcell[4 * i];
                if (wr != scur) {
                    flush_windows();
                    scur = wr;
                }
                if (active) {
                    // every factor is below 2^31 and a double holds it: the product of two such doubles, rounded once, is the
                    // int64 product rounded once - (double)A and (double)B of the definition, bit for bit
                    const int S1 = (int)(hp1 + s1), S2 = (int)(hp2 + s2), SS = (int)(hps + ss), S12 = (int)(hp12 + s12);
                    const int p11 = S1 * S1, p22 = S2 * S2, p12 = S1 * S2;
                    const int vars = 64 * SS - p11 - p22;
                    const int covar = 64 * S12 - p12;
                    const double A = (double)(2 * p12 + 416) * (double)(2 * covar + 235963);
                    const double B = (double)(p11 + p22 + 416) * (double)(vars + 235963);
                    const int q = (int)rint(A / B * 16777216.0);
                    sq += (long long)ww[i - 1] * q;
                }
            }
            hp1 = s1;
            hp2 = s2;
            hps = ss;
            hp12 = s12;
        }
    }
    flush_cells();
    if (SSIM) flush_windows();
}

// ------------------------------------------------------------------ host side
int quality_args(int F, int H, int W, int rows, int cols, bool want_ssim) {
    if (bad_image(F, H, W) || rows < 1 || rows > H || cols < 1 || cols > W) return CP360_ERR_BAD_SHAPE;
    if (want_ssim && (H % 4 != 0 || W % 4 != 0 || H < 8 || W < 8)) return CP360_ERR_BAD_SHAPE;
    if ((double)H * (double)W * 65025.0 * 1024.0 >= 4611686018427387904.0) return CP360_ERR_UNSUPPORTED;     // a cell's sum >= 2^62
    if (big_image(F, H, W) || W > kQMaxW) return CP360_ERR_UNSUPPORTED;
    if (want_ssim && (long long)H * W >= (1LL << 29)) return CP360_ERR_UNSUPPORTED;                          // |ssim_q| <= 2^33 H W
    return CP360_OK;
}

// the tables of K26a in a workspace
struct QTables {
    size_t colcell, rowcell, aw, ww, bytes;
};

QTables quality_tables(int H, int W) {
    QTables t;
    t.colcell = 0;
    t.rowcell = t.colcell + align16((size_t)W * sizeof(int));
    t.aw = t.rowcell + align16((size_t)H * sizeof(int));
    t.ww = t.aw + align16((size_t)H * sizeof(int));
    t.bytes = t.ww + align16((size_t)(H / 4 + 1) * sizeof(int));
    return t;
}

// 256 blocks of columns per workgroup, 64 where a cell can be narrower than a block; chunks of equal width.  Bands of 32 block
// rows (the halo is then 1 / 32), shorter while that leaves the chip fewer than 1024 workgroups
QGeom quality_geom(int F, int H, int W, int rows, int cols) {
    QGeom g;
    g.F = F, g.H = H, g.W = W, g.rows = rows, g.cols = cols;
    const int NB = (W + 3) / 4, NBR = (H + 3) / 4;
    const int cwmax = W / cols >= 4 ? kQThreads : 64;
    g.nchunks = (NB + cwmax - 1) / cwmax;
    g.cw = (NB + g.nchunks - 1) / g.nchunks;
    g.nchunks = (NB + g.cw - 1) / g.cw;
    g.band = 32;
    while (g.band > 4 && (long long)F * g.nchunks * ((NBR + g.band - 1) / g.band) < 1024) g.band >>= 1;
    g.nbands = (NBR + g.band - 1) / g.band;
    return g;
}

}  // namespace

// ------------------------------------------------------------------ C ABI
extern "C" size_t cp360_sphere_quality_work_bytes(int F, int H, int W, int rows, int cols) {
    if (quality_args(F, H, W, rows, cols, false) != CP360_OK) return 0;
    return quality_tables(H, W).bytes;
}

extern "C" int cp360_sphere_quality(const uint8_t* ref, const uint8_t* dist, int F, int H, int W, int rows, int cols,
                                    const int32_t* weights, long long* sse, long long* ssim_q, void* work, size_t work_bytes,
                                    void* stream) {
    if (!ref || !dist || !weights || !sse || !work) return CP360_ERR_NULL;
    int st = quality_args(F, H, W, rows, cols, ssim_q != nullptr);
    if (st != CP360_OK) return st;
    if (((uintptr_t)sse & 7) != 0 || ((uintptr_t)ssim_q & 7) != 0 || ((uintptr_t)weights & 3) != 0) return CP360_ERR_ALIGN;
    const QTables t = quality_tables(H, W);
    st = check_work(work, work_bytes, t.bytes);
    if (st != CP360_OK) return st;
    const QGeom g = quality_geom(F, H, W, rows, cols);
    if ((long long)g.nchunks * g.nbands > 0x7fffffffLL) return CP360_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    char* wk = (char*)work;
    int *colcell = (int*)(wk + t.colcell), *rowcell = (int*)(wk + t.rowcell), *aw = (int*)(wk + t.aw), *ww = (int*)(wk + t.ww);
    const size_t T = (size_t)rows * cols;
    if (hipMemsetAsync(sse, 0, (size_t)F * T * 3 * sizeof(long long), s) != hipSuccess) return CP360_ERR_HIP;
    if (ssim_q && hipMemsetAsync(ssim_q, 0, (size_t)F * T * sizeof(long long), s) != hipSuccess) return CP360_ERR_HIP;
    const int n = H > W ? H : W;
    hipLaunchKernelGGL(quality_tables_kernel, dim3((n + 255) / 256), dim3(256), 0, s, (const int*)weights, colcell, rowcell, aw, ww, H,
                       W, rows, cols);
    CP360_CHECK_HIP();
    const dim3 grid(g.nchunks * g.nbands, F);
    if (ssim_q)
        hipLaunchKernelGGL(quality_kernel<true>, grid, dim3(kQThreads), 0, s, ref, dist, (const int*)colcell, (const int*)rowcell,
                           (const int*)aw, (const int*)ww, (unsigned long long*)sse, (unsigned long long*)ssim_q, g);
    else
        hipLaunchKernelGGL(quality_kernel<false>, grid, dim3(kQThreads), 0, s, ref, dist, (const int*)colcell, (const int*)rowcell,
                           (const int*)aw, (const int*)ww, (unsigned long long*)sse, (unsigned long long*)nullptr, g);
    CP360_CHECK_HIP();
    return CP360_OK;
}
