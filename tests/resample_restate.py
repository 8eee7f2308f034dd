"""The conservative remap on the sphere (K25, csrc/sphere_resample.hip) restated in numpy: the runs and weights in
float64, the forward in float64 (dense matrices) and operation by operation in float32 on weights that are handed in, the adjoint
in float64, and the bound that holds the float32 forward to the float64 one.

Source hs x ws, grid h x w; pixel k of an axis of n spans [k / n, (k + 1) / n].  An axis with n_src > n_dst is conservative: the
run of grid index d is floor(d n_src / n_dst) .. ceil((d + 1) n_src / n_dst) - 1; the column weight is the integer overlap over
ws, the row weight the overlap in z = cos(pi t) over the band's own z range.  Any other axis takes the two bilinear taps of
csrc/sphere.h (position and fraction in float32), the run (i0, i1) with the weights (1 - t, t); columns wrap, rows clamp.
"""
import numpy as np

f32 = np.float32
U = 2.0 ** -24                                # the unit roundoff of float32
# A table entry is float64 rounded once, where the host's cos and numpy's may differ in the last place.  A row weight is a
# quotient of two differences of cosines.  The smallest difference of a source of up to 2048 rows is its polar row's,
# (pi / 2048)^2 / 2 = 1.2e-6; a last place of each of the four cosines (2^-53 near 1) is 4.4e-16 in all, 3.7e-10 of it, which
# is 0.006 of a float32 rounding: allowed for as 2^-7 of one.
TAB_REL = U * (1.0 + 2.0 ** -7)

# (src_hw, hw, F): the cases of tests/test_resample_gpu.py, whose tables tests/test_resample_cpu.py checks
CASES = [
    ((64, 128), (8, 16), 3),                  # integer ratio 8
    ((45, 91), (7, 13), 3),                   # ws is no multiple of 4: 4-byte loads
    ((33, 64), (32, 60), 3),                  # barely finer
    ((16, 32), (5, 9), 3),
    ((100, 37), (3, 36), 3),                  # long row runs, short column runs
    ((40, 16), (8, 32), 3),                   # rows conservative, columns tapped with wrap
    ((6, 96), (12, 24), 3),                   # rows tapped, columns conservative
    ((7, 14), (30, 60), 3),                   # neither axis finer: the bilinear resampler's bits
    ((5, 9), (5, 9), 2),                      # a copy
    ((600, 4500), (512, 37), 2),              # a source wider than one LDS strip: chunks of grid columns
    ((6, 4500), (2, 37), 1),                  # wide, few rows: split and no chunk
    ((64, 2048), (4, 16), 1),                 # one frame, few rows: the columns split over the grid's third dimension
]


def conservative(n_src, n_dst):
    return n_src > n_dst


def run_cap(n_src, n_dst):
    return -(-n_src // n_dst) + 1 if conservative(n_src, n_dst) else 2


def z_edge(k, n):
    """cos(pi k / n), exact at the poles."""
    if k <= 0:
        return 1.0
    if k >= n:
        return -1.0
    return float(np.cos(np.pi * (float(k) / float(n))))


def band(n):
    """float64 [n]: z(y / n) - z((y + 1) / n), the solid angle of row y over 2 pi."""
    return np.array([z_edge(y, n) - z_edge(y + 1, n) for y in range(n)], np.float64)


def taps(n_src, n_dst, axis):
    """The taps of csrc/sphere.h along one axis -> (i0 int64 [n_dst], t float32 [n_dst])."""
    s = ((2.0 * np.arange(n_dst, dtype=np.float64) + 1.0) * n_src / (2.0 * n_dst) - 0.5).astype(f32)
    if axis == 1:
        s = np.where(np.abs(s) <= f32(n_src), s, f32(0))
    else:
        s = np.minimum(np.maximum(s, f32(0)), f32(n_src - 1))
    i0f = np.floor(s)
    t = (s - i0f).astype(f32)
    i0 = i0f.astype(np.int64)
    return (np.mod(i0, n_src) if axis == 1 else i0), t


def axis_tables(n_src, n_dst, axis):
    """-> (start int64 [n_dst], count int64 [n_dst], weights float64 [n_dst, R], overlaps): the weights unrounded on a
    conservative axis (overlaps: the integer column overlaps, None for rows), the float32 tap weights on a tapped one."""
    R = run_cap(n_src, n_dst)
    start, count = np.zeros(n_dst, np.int64), np.zeros(n_dst, np.int64)
    weights = np.zeros((n_dst, R), np.float64)
    overlaps = np.zeros((n_dst, R), np.int64) if axis == 1 else None
    if not conservative(n_src, n_dst):
        i0, t = taps(n_src, n_dst, axis)
        start[:], count[:] = i0, 2
        weights[:, 0], weights[:, 1] = (f32(1) - t).astype(f32), t
        return start, count, weights, None
    for d in range(n_dst):
        lo, hi = (d * n_src) // n_dst, -(-((d + 1) * n_src) // n_dst) - 1
        start[d], count[d] = lo, hi - lo + 1
        bd = z_edge(d, n_dst) - z_edge(d + 1, n_dst)
        for j in range(lo, hi + 1):
            if axis == 1:
                ov = min((j + 1) * n_dst, (d + 1) * n_src) - max(j * n_dst, d * n_src)
                overlaps[d, j - lo] = ov
                weights[d, j - lo] = float(ov) / float(n_src)
            else:
                top = z_edge(j, n_src) if j * n_dst >= d * n_src else z_edge(d, n_dst)
                bot = z_edge(j + 1, n_src) if (j + 1) * n_dst <= (d + 1) * n_src else z_edge(d + 1, n_dst)
                weights[d, j - lo] = (top - bot) / bd
    return start, count, weights, overlaps


def index_of(start, k, n_src, axis):
    """Source index of place k of a run: columns wrap, rows clamp (only a tapped axis ever does either)."""
    i = np.asarray(start, np.int64) + k
    return np.mod(i, n_src) if axis == 1 else np.minimum(i, n_src - 1)


def dense(start, count, weights, n_src, axis, dtype=np.float64):
    """The [n_dst, n_src] matrix of one axis from its tables (two taps on one index add up)."""
    M = np.zeros((len(start), n_src), dtype)
    for d in range(len(start)):
        for k in range(int(count[d])):
            M[d, int(index_of(start[d], k, n_src, axis))] += dtype(weights[d, k])
    return M


def forward64(src, hw):
    """src [F, hs, ws] -> float64 [F, h, w]: the definition in float64, Wy src Wx^T."""
    src = np.asarray(src, np.float64)
    hs, ws = src.shape[1:]
    Wy = dense(*axis_tables(hs, hw[0], 0)[:3], hs, 0)
    Wx = dense(*axis_tables(ws, hw[1], 1)[:3], ws, 1)
    return np.matmul(np.matmul(Wy, src), Wx.T)


def forward_f32(src, ty, tx):
    """src float32 [F, hs, ws], ty / tx = (start, count, weights float32) of the rows / columns -> float32 [F, h, w], operation by
    operation as the kernels: col = 0, col = col + wy * src[r] over the run of y ascending, then out = 0, out = out + wx * col[j]
    over the run of x in run order; every product and every sum rounded to float32 on its own."""
    src = np.ascontiguousarray(src, f32)
    F, hs, ws = src.shape
    (sy, cy, wy), (sx, cx, wx) = ty, tx
    wy, wx = np.asarray(wy, f32), np.asarray(wx, f32)
    h, w = len(sy), len(sx)
    out = np.zeros((F, h, w), f32)
    with np.errstate(invalid='ignore', over='ignore'):
        for y in range(h):
            col = np.zeros((F, ws), f32)
            for k in range(int(cy[y])):
                col = col + wy[y, k] * src[:, int(index_of(sy[y], k, hs, 0)), :]
            o = np.zeros((F, w), f32)
            for k in range(int(np.max(cx))):
                term = o + wx[None, :, k] * col[:, index_of(sx, k, ws, 1)]
                o = np.where((k < np.asarray(cx))[None, :], term, o)
            out[:, y, :] = o
    return out


def forward_bound(n_y, n_x, max_abs):
    """|forward_f32 on the library's tables - forward64| <= this, for run lengths up to n_y and n_x and |src| <= max_abs.

    A term of the double sum is wy wx src.  Against its float64 value it carries the rounding of each weight (TAB_REL apiece; a
    tapped axis has none, its float32 weights are the definition), of the two products, of the n_y - 1 sums its column value
    passes through (the first adds to 0: exact) and of the n_x - 1 sums after it: (1 + TAB_REL)^2 (1 + U)^(n_y + n_x) - 1 at
    most, relative.  The float64 weights of a grid pixel sum to 1 and are positive, so the terms' magnitudes sum to at most
    max_abs.  To first order this is (n_y + n_x + 2) 2^-24 max_abs.  A product may underflow (2^-149 each) and the float64 side
    has roundings of its own (2^-52 where float32 has 2^-24): both are added."""
    rel = (1.0 + TAB_REL) ** 2 * (1.0 + U) ** (n_y + n_x) - 1.0
    return rel * max_abs + n_y * n_x * 2.0 ** -149 + (n_y + n_x + 2) * 2.0 ** -52 * max_abs


def adjoint64(d_dst, src_hw, ty, tx):
    """d_dst [F, h, w], the library's tables -> float64 [F, hs, ws]: Wy^T d_dst Wx with the float32 weights taken to float64."""
    hs, ws = src_hw
    Wy = dense(ty[0], ty[1], np.asarray(ty[2], np.float64), hs, 0)
    Wx = dense(tx[0], tx[1], np.asarray(tx[2], np.float64), ws, 1)
    return np.matmul(np.matmul(Wy.T, np.asarray(d_dst, np.float64)), Wx)


def nonfinite_where(src, ty, tx):
    """bool [F, h, w]: the grid pixels whose runs hold a non-finite source value."""
    bad = ~np.isfinite(np.asarray(src))
    hs, ws = bad.shape[1:]
    My = dense(ty[0], ty[1], np.ones_like(np.asarray(ty[2], np.float64)), hs, 0) > 0
    Mx = dense(tx[0], tx[1], np.ones_like(np.asarray(tx[2], np.float64)), ws, 1) > 0
    return np.matmul(np.matmul(My.astype(np.float64), bad.astype(np.float64)), Mx.astype(np.float64).T) > 0


def sphere_integral(maps):
    """maps [F, h, w] -> float64 [F]: sum_y (z(y / h) - z((y + 1) / h)) / w sum_x maps, the integral over the sphere / 2 pi."""
    maps = np.asarray(maps, np.float64)
    return np.einsum('y,fyx->f', band(maps.shape[1]), maps) / maps.shape[2]
