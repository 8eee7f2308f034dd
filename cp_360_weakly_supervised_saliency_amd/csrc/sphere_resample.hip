// K25: the conservative remap on the sphere and its adjoint - the resampler for maps finer than the grid.  A grid pixel is the
// solid-angle-weighted mean of the source pixels it overlaps: a constant stays a constant, the integral over the sphere is kept,
// every source pixel is read.  sphere_eval.hip's bilinear resampler (four taps, no pre-filter) stays the default of every
// consumer; this one is their opt-in.  The specification is the package's own, DESIGN.md "K25" (7q), restated in
// tests/resample_restate.py.
//
//   Source hs x ws, grid h x w, both equirectangular with the same seam and poles; pixel k of an axis of n spans [k / n, (k + 1) / n].
//   An axis on which the source is finer (n_src > n_dst) is CONSERVATIVE: the run of grid index d is the source indices
//     lo = floor(d n_src / n_dst) .. hi = ceil((d + 1) n_src / n_dst) - 1, at most ceil(n_src / n_dst) + 1 of them;
//     columns  wx = (float)((double)ov / ws), ov = min((j + 1) w, (x + 1) ws) - max(j w, x ws), an integer whose sum over the run is ws
//     rows     wy = (float)(ovy / (z(y / h) - z((y + 1) / h))), z(t) = cos(pi t) with z(0) = 1, z(1) = -1, ovy = z(larger upper
//              edge) - z(smaller lower edge), the edges picked by comparing the fractions as integers
//   any other axis takes sphere_sample's two taps: the position and its fraction t in f32 as sphere.h forms them, the run
//     (i0, i1) with the weights (1 - t, t); columns wrap, rows clamp.
//   forward  col[j] = 0; for r in run(y) ascending: col[j] = col[j] + wy[y, r] * src[r, j];  out = 0; for j in run(x) in run order:
//            out = out + wx[x, j] * col[j] - f32, every product and sum rounded on its own
//   adjoint  d_src[r, j] = sum over the grid rows y whose run holds r of wy[y, r] * (sum over the grid columns x whose run holds j
//            of wx[x, j] * d_dst[y, x]), both sums in f64, rounded once
//
// The tables (start, count, weights per grid index and axis) are made on the host in float64, once per pair of shapes
// (sresample_axis): no kernel does trigonometry.  A caller uploads the plan cp360_sresample_plan_host fills; the kernels clamp
// what they read from it, so that no plan content leads outside src or dst.
//
// Forward launches, one per call, no atomics, no host synchronisation, the order of every sum fixed by the two shapes alone:
//   stream   columns conservative (ws > w): grid (h, F, splits), 256 threads.  A workgroup owns one grid row of one frame (and one
//            range of its columns).  It walks the row's band of source rows once: a lane owns four adjacent source columns per
//            1024-column pass and keeps their vertical sums in registers, eight rows in flight, 16-byte loads (4-byte loads where
//            ws or the pointer is not a multiple of 16 bytes).  The strip of sums goes through LDS (kStrip columns; wider sources
//            in chunks of whole grid columns), then one lane per grid column adds its horizontal run.  A source row on a band's
//            edge is read by two workgroups, nothing else twice.
//   taps     columns tapped, rows conservative (ws <= w, hs > h): one thread per grid pixel walks its two columns' runs itself;
//            the source is no wider than the grid, neighbours share its cache lines.
//   neither axis finer: cp360_seval_resample's launch, its bits.
// Adjoint: grid (ceil(ws / 256), hs, F); one thread per source pixel gathers from the one or two grid rows and columns whose
// runs hold it; a workgroup stays in one source row, so its grid rows are scalar work.
#include "roc.h"

#include <math.h>
#include <string.h>

#pragma clang fp contract(off)

namespace {

constexpr int kMaxRun = 256;                 // the longest run of either axis
constexpr int kStrip = 4096;                 // source columns of one LDS strip (16 KiB)
constexpr int kStripGroups = kStrip / 4 / 256;   // float4 groups a lane owns per strip
constexpr int kRowsInFlight = 8;

// ------------------------------------------------------------------ host: runs and weights of one axis
bool axis_conservative(int n_src, int n_dst) { return n_src > n_dst; }

int axis_run_cap(int n_src, int n_dst) {
    return axis_conservative(n_src, n_dst) ? (int)(((long long)n_src + n_dst - 1) / n_dst) + 1 : 2;
}

double z_edge(long long k, long long n) {    // cos(pi k / n), exact at the poles
    if (k <= 0) return 1.0;
    if (k >= n) return -1.0;
    return cos(3.14159265358979323846 * ((double)k / (double)n));
}

// start, count [n_dst], weights [n_dst, R] zero-padded; rows: axis 0, columns: axis 1
void sresample_axis(int n_src, int n_dst, int axis, int32_t* start, int32_t* count, float* weights) {
    const int R = axis_run_cap(n_src, n_dst);
    const long long ns = n_src, nd = n_dst;
    for (int d = 0; d < n_dst; ++d) {
        float* wrow = weights + (size_t)d * R;
        for (int k = 0; k < R; ++k) wrow[k] = 0.f;
        if (!axis_conservative(n_src, n_dst)) {
            float s = (float)((double)((long long)(2 * (long long)d + 1) * ns) / (double)(2 * nd) - 0.5);
            if (axis == 1) {
                if (!(fabsf(s) <= (float)n_src)) s = 0.f;
            } else {
                s = fminf(fmaxf(s, 0.f), (float)(n_src - 1));
            }
            const float i0f = floorf(s);
            const float t = s - i0f;
            int i0 = (int)i0f;
            if (axis == 1) {
                i0 %= n_src;
                if (i0 < 0) i0 += n_src;
            }
            start[d] = i0;                   // the second tap is start + 1, wrapped (columns) or clamped (rows) by the reader
            count[d] = 2;
            wrow[0] = 1.f - t;
            wrow[1] = t;
            continue;
        }
        const long long lo = (d * ns) / nd, hi = ((d + 1) * ns + nd - 1) / nd - 1;
        start[d] = (int)lo;
        count[d] = (int)(hi - lo + 1);
        const double band = z_edge(d, nd) - z_edge(d + 1, nd);
        for (long long j = lo; j <= hi; ++j) {
            if (axis == 1) {
                const long long a = (j + 1) * nd < (d + 1) * ns ? (j + 1) * nd : (d + 1) * ns;
                const long long b = j * nd > d * ns ? j * nd : d * ns;
                wrow[j - lo] = (float)((double)(a - b) / (double)ns);
            } else {
                // upper edge: the larger of j / ns and d / nd; lower edge: the smaller of (j + 1) / ns and (d + 1) / nd
                const double top = j * nd >= d * ns ? z_edge(j, ns) : z_edge(d, nd);
                const double bot = (j + 1) * nd <= (d + 1) * ns ? z_edge(j + 1, ns) : z_edge(d + 1, nd);
                wrow[j - lo] = (float)((top - bot) / band);
            }
        }
    }
}

// the plan of a pair of shapes: six tables, each 16-byte aligned
struct PlanLayout {
    int Ry, Rx;
    size_t sy, cy, wy, sx, cx, wx, total;
};

PlanLayout plan_layout(int hs, int ws, int h, int w) {
    PlanLayout l;
    l.Ry = axis_run_cap(hs, h);
    l.Rx = axis_run_cap(ws, w);
    l.sy = 0;
    l.cy = l.sy + align16((size_t)h * 4);
    l.wy = l.cy + align16((size_t)h * 4);
    l.sx = l.wy + align16((size_t)h * l.Ry * 4);
    l.cx = l.sx + align16((size_t)w * 4);
    l.wx = l.cx + align16((size_t)w * 4);
    l.total = l.wx + align16((size_t)w * l.Rx * 4);
    return l;
}

struct Plan {
    const int *sy, *cy, *sx, *cx;
    const float *wy, *wx;
    int Ry, Rx;
};

Plan open_plan(const void* plan, const PlanLayout& l) {
    const char* p = (const char*)plan;
    Plan t;
    t.sy = (const int*)(p + l.sy);
    t.cy = (const int*)(p + l.cy);
    t.wy = (const float*)(p + l.wy);
    t.sx = (const int*)(p + l.sx);
    t.cx = (const int*)(p + l.cx);
    t.wx = (const float*)(p + l.wx);
    t.Ry = l.Ry;
    t.Rx = l.Rx;
    return t;
}

// ------------------------------------------------------------------ device: a run as the plan gives it, inside the source whatever it holds
__device__ __forceinline__ void run_of(const int* __restrict__ start, const int* __restrict__ count, int d, int n_src, int R, int& s,
                                       int& c) {
    s = fix_clamp(start[d], 0, n_src - 1);
    c = fix_clamp(count[d], 0, R);
}

__device__ __forceinline__ int row_at(int s, int k, int hs) { return s + k < hs ? s + k : hs - 1; }    // rows clamp
__device__ __forceinline__ int col_at(int s, int k, int ws) { return (s + k) % ws; }                   // columns wrap

// ------------------------------------------------------------------ forward, the stream
// grid (h, F, splits), 256 threads; cols_per_block grid columns per workgroup, cols_per_chunk of them per LDS strip
template <bool VEC>
__global__ __launch_bounds__(256) void sresample_stream_kernel(const float* __restrict__ src, int hs, int ws, float* __restrict__ dst,
                                                               int h, int w, Plan t, int cols_per_block, int cols_per_chunk) {
    __shared__ float strip[kStrip];
    const int tid = threadIdx.x, y = blockIdx.x, f = blockIdx.y;
    const float* img = src + (size_t)f * hs * ws;
    float* out = dst + ((size_t)f * h + y) * w;
    int ys, yc;
    run_of(t.sy, t.cy, y, hs, t.Ry, ys, yc);
    const float* wy = t.wy + (size_t)y * t.Ry;
    const int xb = blockIdx.z * cols_per_block;
    const int xe = xb + cols_per_block < w ? xb + cols_per_block : w;
    for (int x0 = xb; x0 < xe; x0 += cols_per_chunk) {
        const int x1 = x0 + cols_per_chunk < xe ? x0 + cols_per_chunk : xe;
        int s0, c0, s1, c1;
        run_of(t.sx, t.cx, x0, ws, t.Rx, s0, c0);
        run_of(t.sx, t.cx, x1 - 1, ws, t.Rx, s1, c1);
        const int base = s0 & ~3;                                      // the strip starts on a 16-byte boundary of the row
        int end = s1 + c1 < ws ? s1 + c1 : ws;                         // one past the last source column of the chunk
        if (end > base + kStrip) end = base + kStrip;
#pragma unroll
        for (int g = 0; g < kStripGroups; ++g) {
            const int c = base + (g * 256 + tid) * 4;
            if (c >= end) continue;
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            int k = 0;
            if (VEC) {
                for (; k + kRowsInFlight <= yc; k += kRowsInFlight) {
                    float4 v[kRowsInFlight];
#pragma unroll
                    for (int u = 0; u < kRowsInFlight; ++u)
                        v[u] = *(const float4*)(img + (size_t)row_at(ys, k + u, hs) * ws + c);
#pragma unroll
                    for (int u = 0; u < kRowsInFlight; ++u) {
                        const float wr = wy[k + u];
                        acc.x = acc.x + wr * v[u].x;
                        acc.y = acc.y + wr * v[u].y;
                        acc.z = acc.z + wr * v[u].z;
                        acc.w = acc.w + wr * v[u].w;
                    }
                }
                for (; k < yc; ++k) {
                    const float4 v = *(const float4*)(img + (size_t)row_at(ys, k, hs) * ws + c);
                    const float wr = wy[k];
                    acc.x = acc.x + wr * v.x;
                    acc.y = acc.y + wr * v.y;
                    acc.z = acc.z + wr * v.z;
                    acc.w = acc.w + wr * v.w;
                }
            } else {
                const bool in1 = c + 1 < end, in2 = c + 2 < end, in3 = c + 3 < end;
                for (; k < yc; ++k) {
                    const float* p = img + (size_t)row_at(ys, k, hs) * ws + c;
                    const float wr = wy[k];
                    acc.x = acc.x + wr * p[0];
                    if (in1) acc.y = acc.y + wr * p[1];
                    if (in2) acc.z = acc.z + wr * p[2];
                    if (in3) acc.w = acc.w + wr * p[3];
                }
            }
            *(float4*)(strip + (c - base)) = acc;
        }
        __syncthreads();
        for (int x = x0 + tid; x < x1; x += 256) {
            int xs, xc;
            run_of(t.sx, t.cx, x, ws, t.Rx, xs, xc);
            const float* wx = t.wx + (size_t)x * t.Rx;
            float o = 0.f;
            for (int k = 0; k < xc; ++k) {
                const int j = xs + k - base;
                if (j < 0 || j >= end - base) break;                   // only a plan that is not this pair's
                o = o + wx[k] * strip[j];
            }
            out[x] = o;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------ forward, the taps: grid (ceil(h w / 256), F), a thread per grid pixel
__global__ __launch_bounds__(256) void sresample_taps_kernel(const float* __restrict__ src, int hs, int ws, float* __restrict__ dst,
                                                             int h, int w, Plan t) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= h * w) return;
    const int f = blockIdx.y;
    const float* img = src + (size_t)f * hs * ws;
    const int y = i / w, x = i - y * w;
    int ys, yc, xs, xc;
    run_of(t.sy, t.cy, y, hs, t.Ry, ys, yc);
    run_of(t.sx, t.cx, x, ws, t.Rx, xs, xc);
    const float* wy = t.wy + (size_t)y * t.Ry;
    const float* wx = t.wx + (size_t)x * t.Rx;
    float o = 0.f;
    for (int kx = 0; kx < xc; ++kx) {
        const int j = col_at(xs, kx, ws);
        float col = 0.f;
        for (int ky = 0; ky < yc; ++ky) col = col + wy[ky] * img[(size_t)row_at(ys, ky, hs) * ws + j];
        o = o + wx[kx] * col;
    }
    dst[(size_t)f * h * w + i] = o;
}

// ------------------------------------------------------------------ adjoint: grid (ceil(ws / 256), hs, F), a thread per source pixel
// the grid indices that may hold source index k in their run: exact on a conservative axis (SMALL: k n + n_src < 2^31, the
// division in 32 bits), suploss.hip's sup_span (two indices of margin; may leave 0 .. n - 1) on a tapped one
template <bool SMALL>
__device__ __forceinline__ void adj_span(int k, int n, int ns, int& lo, int& hi) {
    if (ns > n) {
        if (SMALL) {
            lo = (int)(((unsigned)k * (unsigned)n) / (unsigned)ns);
            hi = (int)((((unsigned)k + 1u) * (unsigned)n + (unsigned)ns - 1u) / (unsigned)ns) - 1;
        } else {
            lo = (int)(((long long)k * n) / ns);
            hi = (int)((((long long)k + 1) * n + ns - 1) / ns) - 1;
        }
        return;
    }
    const double scale = (double)(2 * (long long)n) / (double)ns;
    lo = (int)floor((((double)k - 0.5) * scale - 1.0) * 0.5) - 2;
    hi = (int)ceil((((double)k + 1.5) * scale - 1.0) * 0.5) + 2;
}

// A workgroup stays in one source row: its grid rows and their weights are the same in every lane (scalar work), a lane finds
// the one or two grid columns of its own source column.
template <bool SMALL>
__global__ __launch_bounds__(256) void sresample_adjoint_kernel(const float* __restrict__ dd, int h, int w, float* __restrict__ ds, int hs,
                                                                int ws, Plan t) {
    const int j = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y, f = blockIdx.z;
    if (j >= ws) return;
    dd += (size_t)f * h * w;
    int ylo, yhi, xlo, xhi;
    adj_span<false>(r, h, hs, ylo, yhi);
    adj_span<SMALL>(j, w, ws, xlo, xhi);
    if (ylo < 0 || (hs <= h && r == 0)) ylo = 0;                       // rows clamp: the first and the last source row collect
    if (yhi > h - 1 || (hs <= h && r == hs - 1)) yhi = h - 1;          // from every grid row beyond them
    if ((long long)xhi - xlo + 1 >= w) {                               // the span covers the circle: every column once
        xlo = 0;
        xhi = w - 1;
    }
    double acc = 0.0;
    for (int y = ylo; y <= yhi; ++y) {
        int ys, yc;
        run_of(t.sy, t.cy, y, hs, t.Ry, ys, yc);
        const float* wy = t.wy + (size_t)y * t.Ry;
        // where r sits in the run of y: one place on a conservative axis, either tap on a tapped one
        int k0 = r - ys, k1 = r - ys + 1;
        if (hs <= h) {
            k0 = 0;
            k1 = 2;
        }
        for (int ky = k0 < 0 ? 0 : k0; ky < k1 && ky < yc; ++ky) {
            if (row_at(ys, ky, hs) != r) continue;
            const double wr = (double)wy[ky];
            double inner = 0.0;
            for (int xu = xlo; xu <= xhi; ++xu) {
                const int x = xu >= 0 && xu < w ? xu : ((xu % w) + w) % w;    // columns wrap
                int xs, xc;
                run_of(t.sx, t.cx, x, ws, t.Rx, xs, xc);
                const float* wx = t.wx + (size_t)x * t.Rx;
                int j0 = j - xs, j1 = j - xs + 1;
                if (ws <= w) {
                    j0 = 0;
                    j1 = 2;
                }
                for (int kx = j0 < 0 ? 0 : j0; kx < j1 && kx < xc; ++kx)
                    if (col_at(xs, kx, ws) == j) inner += (double)wx[kx] * (double)dd[(size_t)y * w + x];
            }
            acc += wr * inner;
        }
    }
    ds[((size_t)f * hs + r) * ws + j] = (float)acc;
}

// the checks the entry points share, cp360_seval_resample's limits; F = 0 is valid (nothing to launch)
int sresample_args(int F, int hs, int ws, int h, int w) {
    if (F < 0 || bad_image(1, hs, ws) || bad_image(1, h, w)) return CP360_ERR_BAD_SHAPE;
    const int st = roc_args(F > 0 ? F : 1, h, w);
    if (st != CP360_OK) return st;
    if (big_image(F, hs, ws)) return CP360_ERR_UNSUPPORTED;
    if (axis_run_cap(hs, h) > kMaxRun || axis_run_cap(ws, w) > kMaxRun) return CP360_ERR_UNSUPPORTED;
    return CP360_OK;
}

}  // namespace

// ------------------------------------------------------------------ C ABI
extern "C" int cp360_sresample_run_cap(int n_src, int n_dst) {
    if (n_src < 1 || n_dst < 1) return 0;
    return axis_run_cap(n_src, n_dst);
}

extern "C" int cp360_sresample_axis_host(int n_src, int n_dst, int axis, int32_t* start, int32_t* count, float* weights) {
    if (!start || !count || !weights) return CP360_ERR_NULL;
    if (n_src < 1 || n_dst < 1 || (axis != 0 && axis != 1)) return CP360_ERR_BAD_SHAPE;
    if (n_src > (1 << 28) || n_dst > (1 << 21) || axis_run_cap(n_src, n_dst) > kMaxRun) return CP360_ERR_UNSUPPORTED;
    sresample_axis(n_src, n_dst, axis, start, count, weights);
    return CP360_OK;
}

extern "C" size_t cp360_sresample_plan_bytes(int hs, int ws, int h, int w) {
    if (sresample_args(1, hs, ws, h, w) != CP360_OK) return 0;
    return plan_layout(hs, ws, h, w).total;
}

extern "C" int cp360_sresample_plan_host(int hs, int ws, int h, int w, void* plan, size_t plan_bytes) {
    if (!plan) return CP360_ERR_NULL;
    int st = sresample_args(1, hs, ws, h, w);
    if (st != CP360_OK) return st;
    const PlanLayout l = plan_layout(hs, ws, h, w);
    st = check_work(plan, plan_bytes, l.total);
    if (st != CP360_OK) return st;
    memset(plan, 0, l.total);
    char* p = (char*)plan;
    sresample_axis(hs, h, 0, (int32_t*)(p + l.sy), (int32_t*)(p + l.cy), (float*)(p + l.wy));
    sresample_axis(ws, w, 1, (int32_t*)(p + l.sx), (int32_t*)(p + l.cx), (float*)(p + l.wx));
    return CP360_OK;
}

extern "C" int cp360_sresample_forward(const float* src, int F, int hs, int ws, float* dst, int h, int w, const void* plan,
                                       size_t plan_bytes, void* stream) {
    if (!plan || ((!src || !dst) && F != 0)) return CP360_ERR_NULL;
    int st = sresample_args(F, hs, ws, h, w);
    if (st != CP360_OK) return st;
    if (((uintptr_t)src & 3) != 0 || ((uintptr_t)dst & 3) != 0) return CP360_ERR_ALIGN;
    const PlanLayout l = plan_layout(hs, ws, h, w);
    st = check_work(plan, plan_bytes, l.total);
    if (st != CP360_OK || F == 0) return st;
    if (hs <= h && ws <= w) return cp360_seval_resample(src, F, hs, ws, dst, h, w, stream);   // neither axis finer: its bits
    const Plan t = open_plan(plan, l);
    hipStream_t s = (hipStream_t)stream;
    if (ws <= w) {
        hipLaunchKernelGGL(sresample_taps_kernel, dim3((h * w + 255) / 256, F), dim3(256), 0, s, src, hs, ws, dst, h, w, t);
        CP360_CHECK_HIP();
        return CP360_OK;
    }
    // whole grid columns per strip: n columns span at most n ws / w + 2 source columns, and up to 3 more for the alignment
    int cols_per_chunk = (int)(((long long)(kStrip - 6) * w) / ws);
    if (cols_per_chunk < 1) cols_per_chunk = 1;                        // cannot be: a run is at most kMaxRun
    // few rows and frames: split the columns until about four workgroups per CU are in flight, each at least 512 source columns wide
    long long splits = (1024 + (long long)h * F - 1) / ((long long)h * F);
    if (splits > ws / 512) splits = ws / 512;
    if (splits > w) splits = w;
    if (splits < 1) splits = 1;
    const int cols_per_block = (int)((w + splits - 1) / splits);
    const dim3 grid(h, F, (w + cols_per_block - 1) / cols_per_block);
    if (ws % 4 == 0 && aligned16(src))
        hipLaunchKernelGGL(sresample_stream_kernel<true>, grid, dim3(256), 0, s, src, hs, ws, dst, h, w, t, cols_per_block, cols_per_chunk);
    else
        hipLaunchKernelGGL(sresample_stream_kernel<false>, grid, dim3(256), 0, s, src, hs, ws, dst, h, w, t, cols_per_block, cols_per_chunk);
    CP360_CHECK_HIP();
    return CP360_OK;
}

extern "C" int cp360_sresample_adjoint(const float* d_dst, int F, int h, int w, float* d_src, int hs, int ws, const void* plan,
                                       size_t plan_bytes, void* stream) {
    if (!plan || ((!d_dst || !d_src) && F != 0)) return CP360_ERR_NULL;
    int st = sresample_args(F, hs, ws, h, w);
    if (st != CP360_OK) return st;
    if (((uintptr_t)d_dst & 3) != 0 || ((uintptr_t)d_src & 3) != 0) return CP360_ERR_ALIGN;
    const PlanLayout l = plan_layout(hs, ws, h, w);
    st = check_work(plan, plan_bytes, l.total);
    if (st != CP360_OK || F == 0) return st;
    const dim3 grid((ws + 255) / 256, hs, F);
    if ((long long)ws * w + ws < (1LL << 31))
        hipLaunchKernelGGL(sresample_adjoint_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, d_dst, h, w, d_src, hs, ws,
                           open_plan(plan, l));
    else
        hipLaunchKernelGGL(sresample_adjoint_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, d_dst, h, w, d_src, hs, ws,
                           open_plan(plan, l));
    CP360_CHECK_HIP();
    return CP360_OK;
}
