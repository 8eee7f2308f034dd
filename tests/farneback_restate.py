"""numpy restatement of the package's Farneback optical flow (DESIGN.md "K10": the specification the HIP kernels of
csrc/optflow.hip implement), statement by statement, with a ``dtype`` argument:

  * ``np.float64`` is the reference of the GPU tests;
  * ``np.float32`` runs the same statements in float32 and is used only to measure the reference's own float32 sensitivity
    (the end-to-end tolerance is a multiple of max|restate(f32) - restate(f64)|).

It imports nothing from the package.  cv2 is not a test dependency, so this pins the specification (OpenCV's implementation as
recalled), not cv2 itself.  All convolutions are correlations; cvRound is round-half-to-even.  The tables that the
specification rounds to float32 for the kernels (Gaussian taps, g / xg / xxg, the four ig constants) are rounded here too
(``round32=True``), so both sides start from the same numbers; ``round32=False`` keeps them in double for the analytic
known-answer test of the expansion.

Sign convention: prev(y, x) ~ next(y + flow[y, x, 1], x + flow[y, x, 0]); flow is [H, W, 2] = (dx, dy) in pixels.
"""
import numpy as np

BORDER = (0.14, 0.14, 0.4472, 0.4472, 0.4472)
MIN_SIZE = 32


def cv_round(v):
    return int(np.rint(v))                      # round half to even


# ----------------------------------------------------------------------------- 0. frames to gray
def gray_from_rgb(resized_u8):
    """u8 [..., 3] as the video reader delivers it, ALREADY resized (the resize acts per channel, so it commutes with the
    reversal) -> f32 gray 0..255: channels reversed, then cv2's BGR2GRAY arithmetic on that array."""
    c = resized_u8[..., ::-1].astype(np.int64)
    return ((c[..., 0] * 1868 + c[..., 1] * 9617 + c[..., 2] * 4899 + 8192) >> 14).astype(np.float32)


# ----------------------------------------------------------------------------- 1. pyramid
def level_geometry(H, W, pyr_scale=0.5, levels=7):
    """[(h, w, ksz, sigma)] of levels k = 0 (full size) .. L."""
    k, scale = 0, 1.0
    while k < levels:
        scale *= pyr_scale
        if W * scale < MIN_SIZE or H * scale < MIN_SIZE:
            break
        k += 1
    out = []
    for kk in range(k + 1):
        scale = 1.0
        for _ in range(kk):
            scale *= pyr_scale
        sigma = (1.0 / scale - 1.0) * 0.5
        ksz = max(cv_round(sigma * 5) | 1, 3)
        out.append((cv_round(H * scale), cv_round(W * scale), ksz, sigma))
    return out


def gauss_kernel(ksz, sigma, round32=True):
    if sigma <= 0:
        assert ksz == 3
        return np.array([0.25, 0.5, 0.25])
    x = np.arange(ksz, dtype=np.float64) - ksz // 2
    g = np.exp(-x * x / (2.0 * sigma * sigma))
    g = g / g.sum()
    return g.astype(np.float32).astype(np.float64) if round32 else g


def reflect101(i, n):
    """Border reflect-101 folded as often as it takes (an image smaller than the kernel): period 2 (n - 1)."""
    i = np.asarray(i)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = np.mod(i, p)
    return np.where(i < n, i, p - i)


def _lin_axis(n_src, n_dst, dtype):
    """Half-pixel centres, edge clamp (the arithmetic of the library's linear resize): i0, i1, fraction."""
    d = np.arange(n_dst, dtype=np.float64)
    f = (d + 0.5) * (float(n_src) / float(n_dst)) - 0.5
    i = np.floor(f).astype(np.int64)
    t = f - i
    if dtype == np.float32:
        t = t.astype(np.float32)
    lo, hi = i < 0, i >= n_src - 1
    i = np.where(lo, 0, np.where(hi, n_src - 1, i))
    t = np.where(lo | hi, 0, t).astype(dtype)
    return i, np.minimum(i + 1, n_src - 1), t


def resize_linear(img, dh, dw, dtype=np.float64):
    """[h, w, ...] -> [dh, dw, ...]: rows first, then the vertical blend."""
    img = np.asarray(img, dtype=dtype)
    y0, y1, fy = _lin_axis(img.shape[0], dh, dtype)
    x0, x1, fx = _lin_axis(img.shape[1], dw, dtype)
    extra = (1,) * (img.ndim - 2)
    fx = fx.reshape((1, dw) + extra)
    fy = fy.reshape((dh, 1) + extra)
    one = dtype(1)
    top = img[y0][:, x0] * (one - fx) + img[y0][:, x1] * fx
    bot = img[y1][:, x0] * (one - fx) + img[y1][:, x1] * fx
    return (top * (one - fy) + bot * fy).astype(dtype)


def gauss_blur(img, ksz, sigma, dtype=np.float64):
    """ksz x ksz separable Gaussian, border reflect-101, horizontal pass first."""
    img = np.asarray(img, dtype=dtype)
    taps = gauss_kernel(ksz, sigma).astype(dtype)
    h, w = img.shape
    r = ksz // 2
    acc = np.zeros_like(img)
    for k in range(ksz):
        acc = acc + taps[k] * img[:, reflect101(np.arange(w) + k - r, w)]
    out = np.zeros_like(img)
    for k in range(ksz):
        out = out + taps[k] * acc[reflect101(np.arange(h) + k - r, h), :]
    return out


def pyr_level(gray, ksz, sigma, lh, lw, dtype=np.float64):
    return resize_linear(gauss_blur(gray, ksz, sigma, dtype), lh, lw, dtype)


def flow_upsample(flow, nh, nw, mul, dtype=np.float64):
    return (resize_linear(flow, nh, nw, dtype) * dtype(np.float32(mul))).astype(dtype)


# ----------------------------------------------------------------------------- 2. polynomial expansion
def poly_tables(n, sigma, round32=True):
    """g, xg, xxg [2n + 1] and ig = (ig11, ig03, ig33, ig55), float64 arrays (values rounded through float32 if round32)."""
    x = np.arange(-n, n + 1, dtype=np.float64)
    g = np.exp(-x * x / (2.0 * sigma * sigma))
    g = g / g.sum()
    yy, xx = np.meshgrid(x, x, indexing='ij')
    wgt = np.outer(g, g)
    basis = np.stack([np.ones_like(xx), xx, yy, xx * xx, yy * yy, xx * yy])          # (1, x, y, x^2, y^2, xy)
    G = np.einsum('yx,iyx,jyx->ij', wgt, basis, basis)
    inv = np.linalg.inv(G)
    ig = np.array([inv[1, 1], inv[0, 3], inv[3, 3], inv[5, 5]])
    xg, xxg = x * g, x * x * g
    if round32:
        g, xg, xxg, ig = (a.astype(np.float32).astype(np.float64) for a in (g, xg, xxg, ig))
    return g, xg, xxg, ig


def poly_exp(img, n=5, sigma=1.2, dtype=np.float64, round32=True, tables=None):
    """[h, w] -> R [5, h, w]: the local coefficients of [y, x, y^2, x^2, xy]; rows and columns replicate-clamped.
    ``tables`` replaces poly_tables(n, sigma) (the tests bound the rounding error with the tables' absolute values)."""
    img = np.asarray(img, dtype=dtype)
    g, xg, xxg, ig = (np.asarray(a).astype(dtype) for a in (tables or poly_tables(n, sigma, round32)))
    h, w = img.shape
    r0, r1, r2 = (np.zeros_like(img) for _ in range(3))
    for k in range(2 * n + 1):
        v = img[np.clip(np.arange(h) + k - n, 0, h - 1), :]
        r0, r1, r2 = r0 + g[k] * v, r1 + xg[k] * v, r2 + xxg[k] * v
    b1, b2, b3, b4, b5, b6 = (np.zeros_like(img) for _ in range(6))
    for k in range(2 * n + 1):
        c = np.clip(np.arange(w) + k - n, 0, w - 1)
        v0, v1, v2 = r0[:, c], r1[:, c], r2[:, c]
        b1, b2, b3 = b1 + g[k] * v0, b2 + xg[k] * v0, b3 + g[k] * v1
        b4, b5, b6 = b4 + xxg[k] * v0, b5 + g[k] * v2, b6 + xg[k] * v1
    ig11, ig03, ig33, ig55 = ig
    return np.stack([b3 * ig11, b2 * ig11, b1 * ig03 + b5 * ig33, b1 * ig03 + b4 * ig33, b6 * ig55]).astype(dtype)


# ----------------------------------------------------------------------------- 3. matrices
def sample_positions(flow, dtype=np.float64):
    """fx, fy [h, w] of the sample of next's expansion, and the in-bounds mask of the specification."""
    flow = np.asarray(flow, dtype=dtype)
    h, w = flow.shape[:2]
    fx = np.arange(w, dtype=dtype)[None, :] + flow[..., 0]
    fy = np.arange(h, dtype=dtype)[:, None] + flow[..., 1]
    x1, y1 = np.floor(fx), np.floor(fy)
    inside = (x1 >= 0) & (x1 < w - 1) & (y1 >= 0) & (y1 < h - 1)
    return fx, fy, inside


def border_scale(h, w, dtype=np.float64):
    def axis(n):
        s = np.ones(n, dtype=dtype)
        for i in range(n):
            if i < 5:
                s[i] = s[i] * dtype(np.float32(BORDER[i]))
            if i >= n - 5:
                s[i] = s[i] * dtype(np.float32(BORDER[n - 1 - i]))
        return s
    sx, sy = axis(w), axis(h)
    return (sx[None, :] * sy[:, None]).astype(dtype)


def matrices(R0, R1, flow, dtype=np.float64):
    """R0 (prev), R1 (next) [5, h, w], flow [h, w, 2] -> M [5, h, w]."""
    R0, R1, flow = (np.asarray(a, dtype=dtype) for a in (R0, R1, flow))
    h, w = flow.shape[:2]
    dx, dy = flow[..., 0], flow[..., 1]
    fx, fy, inside = sample_positions(flow, dtype)
    # a NaN position compares false with every bound, so it is outside and its taps are never used: any valid index serves
    x1 = np.clip(np.nan_to_num(np.floor(fx), nan=0.0), 0, max(w - 2, 0)).astype(np.int64)
    y1 = np.clip(np.nan_to_num(np.floor(fy), nan=0.0), 0, max(h - 2, 0)).astype(np.int64)
    x2, y2 = np.minimum(x1 + 1, w - 1), np.minimum(y1 + 1, h - 1)
    ax, ay = fx - np.floor(fx), fy - np.floor(fy)
    one, half, quarter = dtype(1), dtype(0.5), dtype(0.25)
    w00, w01, w10, w11 = (one - ax) * (one - ay), ax * (one - ay), (one - ax) * ay, ax * ay
    S = w00 * R1[:, y1, x1] + w01 * R1[:, y1, x2] + w10 * R1[:, y2, x1] + w11 * R1[:, y2, x2]
    zero = np.zeros_like(dx)
    r2 = np.where(inside, S[0], zero)
    r3 = np.where(inside, S[1], zero)
    r4 = np.where(inside, (R0[2] + S[2]) * half, R0[2])
    r5 = np.where(inside, (R0[3] + S[3]) * half, R0[3])
    r6 = np.where(inside, (R0[4] + S[4]) * quarter, R0[4] * half)
    r2 = (R0[0] - r2) * half
    r3 = (R0[1] - r3) * half
    r2 = r2 + (r4 * dy + r6 * dx)
    r3 = r3 + (r6 * dy + r5 * dx)
    sc = border_scale(h, w, dtype)
    r2, r3, r4, r5, r6 = r2 * sc, r3 * sc, r4 * sc, r5 * sc, r6 * sc
    return np.stack([r4 * r4 + r6 * r6, (r4 + r5) * r6, r5 * r5 + r6 * r6, r4 * r2 + r6 * r3, r6 * r2 + r5 * r3]).astype(dtype)


# ----------------------------------------------------------------------------- 4. blur and solve
def box_mean(M, winsize, dtype=np.float64):
    """[..., h, w] -> the (2m+1)^2 box mean, rows and columns replicate-clamped."""
    M = np.asarray(M, dtype=dtype)
    m = winsize // 2
    h, w = M.shape[-2:]
    v = np.zeros_like(M)
    for k in range(2 * m + 1):
        v = v + M[..., np.clip(np.arange(h) + k - m, 0, h - 1), :]
    s = np.zeros_like(M)
    for k in range(2 * m + 1):
        s = s + v[..., np.clip(np.arange(w) + k - m, 0, w - 1)]
    area = (2 * m + 1) ** 2
    return s / area if dtype == np.float64 else (s * np.float32(1.0 / area)).astype(dtype)


def blur_solve(M, winsize=15, dtype=np.float64, want_cond=False):
    """M [5, h, w] -> flow [h, w, 2]; want_cond: also |g11 g22| / |det + 1e-3|, the conditioning of the 2 x 2 solve."""
    if winsize % 2 == 0:
        raise ValueError("winsize must be odd")
    g11, g12, g22, h1, h2 = box_mean(M, winsize, dtype)
    det = g11 * g22 - g12 * g12 + dtype(np.float32(1e-3))
    idet = dtype(1) / det
    flow = np.stack([(g11 * h2 - g12 * h1) * idet, (g22 * h1 - g12 * h2) * idet], axis=-1).astype(dtype)
    if want_cond:
        return flow, np.abs(g11 * g22) / np.abs(det), (g11, g12, g22)
    return flow


# ----------------------------------------------------------------------------- 5. the levels
def farneback(gray, pyr_scale=0.5, levels=7, winsize=15, iterations=3, poly_n=5, poly_sigma=1.2, flags=0, dtype=np.float64,
              trace=None):
    """gray [F + 1, H, W] (0..255) -> flow [F, H, W, 2].  trace (a list): one entry per (level k, pair, iteration) =
    (k, pair, iteration, (g11, g12, g22)) of the blurred system, for the conditioning asserts of the tests."""
    if flags != 0:
        raise ValueError("flags other than 0 are not supported")
    if winsize % 2 == 0:
        raise ValueError("winsize must be odd")
    gray = np.asarray(gray, dtype=dtype)
    F, H, W = gray.shape[0] - 1, gray.shape[1], gray.shape[2]
    geo = level_geometry(H, W, pyr_scale, levels)
    flows = None
    for k in range(len(geo) - 1, -1, -1):
        h, w, ksz, sigma = geo[k]
        Rs = [poly_exp(pyr_level(g, ksz, sigma, h, w, dtype), poly_n, poly_sigma, dtype) for g in gray]
        new = []
        for p in range(F):
            fl = np.zeros((h, w, 2), dtype) if flows is None else flow_upsample(flows[p], h, w, 1.0 / pyr_scale, dtype)
            for it in range(iterations):
                M = matrices(Rs[p], Rs[p + 1], fl, dtype)
                fl, _, gs = blur_solve(M, winsize, dtype, want_cond=True)
                if trace is not None:
                    trace.append((k, p, it, gs))
            new.append(fl)
        flows = new
    return np.stack(flows)


# ----------------------------------------------------------------------------- 6. absflow
def absflow(flow):
    """The first return value of the reference's calcOpticalFlow, in the flow's own dtype as numpy computes it."""
    a = np.sqrt(flow[:, :, 0] ** 2 + flow[:, :, 1] ** 2)
    a = a - np.min(a)
    a = a / np.max(a)
    a[a < (np.mean(a) - 1.5 * np.std(a))] = 0
    return a
