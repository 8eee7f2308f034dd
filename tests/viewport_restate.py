"""Float64 numpy restatement of the viewport pilot (K12, csrc/viewport.hip and utils/viewport.py; the specification is DESIGN.md
"K12").  Geometry, tables and pix are K11's (tests/stabilize_restate.py).

A camera is R [3, 3], camera-to-world, with the columns (forward, up, right): R = I looks along dir of the panorama's centre,
(1, 0, 0), with up +y and right +z.  tx = tan(hfov / 2), ty = tx h / w.

    render   view pixel (i, j): u = ((2 i + 1) / w - 1) tx, v = (1 - (2 j + 1) / h) ty, r = 1 / sqrt((1 + v v) + u u),
             d = (r, v r, u r), q = R d, out = bilinear(frame, pix(q)): columns wrap, rows clamp
    outline  panorama pixel (x, y): d = R^T dir(x, y) = (d_f, d_u, d_r), u = d_r / d_f, v = d_u / d_f, b = border_px 2 tx / w;
             border <=> d_f > 0, |u| <= tx, |v| <= ty and not (|u| <= tx - b and |v| <= ty - b)
    smooth   out_i = sum_j a_j s_j e_ij / sum_j a_j e_ij, e_ij = exp(kappa (p_i . p_j - 1)), kappa = 1 / sigma^2, a_j = cos phi_j
    peak     idx = argmax of the smoothed map (lowest index on ties), p* = dir(idx), c = sum_j a_j s_j e(p*, p_j) p_j, dir = c / |c|

``dtype=np.float32`` evaluates every per-pixel term in float32, operation by operation as the kernels do, and keeps the sums in
float64: d32 = max|restate(float32) - restate(float64)| is the unit of the GPU tests' bounds, as for K11.  Nothing here imports
the code under test.
"""
import numpy as np

from tests.stabilize_restate import _pixel_dirs, _rotate, pix, rot, tables, texture  # noqa: F401  (rot, texture: for the tests)


def view_tangents(hw, hfov_deg, dtype=np.float64):
    """(tx, ty) = (tan(hfov / 2), tan(hfov / 2) h / w): float64 values rounded once to dtype."""
    h, w = hw
    t = np.tan(0.5 * np.deg2rad(float(hfov_deg)))
    return dtype(t), dtype(t * h / w)


# ----------------------------------------------------------------------------- render
def view_rays(hw, hfov_deg, dtype=np.float64):
    """The unit ray of every view pixel in the camera's (forward, up, right) basis: three [h, w] arrays."""
    h, w = hw
    tx, ty = view_tangents(hw, hfov_deg, dtype)
    one = dtype(1)
    u = ((2 * np.arange(w) + 1).astype(dtype) / dtype(w) - one) * tx
    v = (one - (2 * np.arange(h) + 1).astype(dtype) / dtype(h)) * ty
    u, v = np.broadcast_to(u[None, :], (h, w)), np.broadcast_to(v[:, None], (h, w))
    r = one / np.sqrt((one + v * v) + u * u)
    return r, v * r, u * r


def sample_positions(R, hw, hfov_deg, H, W, dtype=np.float64):
    """The sample position pix(R d) of every view pixel on the H x W panorama: (sx, sy) [h, w]; sy clamped to 0 .. H - 1, a
    non-finite position moved inside the frame."""
    f, up, rt = view_rays(hw, hfov_deg, dtype)
    with np.errstate(invalid='ignore'):
        sx, sy = pix(np.stack(_rotate(R, f, up, rt, dtype), -1), H, W, dtype)
        sx = np.where(np.abs(sx) <= dtype(W), sx, dtype(0))
        sy = np.where(np.isnan(sy), dtype(0), np.minimum(np.maximum(sy, dtype(0)), dtype(H - 1)))
    return sx, sy


def bilinear(img, sx, sy, dtype=np.float64):
    """img [H, W, C] at the positions (sx, sy): four taps, columns wrap modulo W, rows clamp, top + ty (bot - top)."""
    H, W = img.shape[:2]
    x0f, y0f = np.floor(sx), np.floor(sy)
    tx, ty = (sx - x0f)[..., None], (sy - y0f)[..., None]
    x0 = np.mod(x0f.astype(np.int64), W)
    x1 = np.mod(x0 + 1, W)
    y0 = y0f.astype(np.int64)
    y1 = np.minimum(y0 + 1, H - 1)
    img = img.astype(dtype)
    v00, v01, v10, v11 = img[y0, x0], img[y0, x1], img[y1, x0], img[y1, x1]
    top = v00 + tx * (v01 - v00)
    bot = v10 + tx * (v11 - v10)
    return top + ty * (bot - top)


def render(frames, R, hw, hfov_deg, dtype=np.float64, raw=False):
    """frames u8 or float [N, H, W, C], R [N, 3, 3] -> the views [N, h, w, C].  Float frames return dtype; u8 frames round half
    to even (raw=True: the values before rounding, in dtype)."""
    frames = np.asarray(frames)
    N, H, W, C = frames.shape
    R = np.broadcast_to(np.asarray(R, np.float64), (N, 3, 3))
    out = np.empty((N, hw[0], hw[1], C), dtype)
    for n in range(N):
        sx, sy = sample_positions(R[n], hw, hfov_deg, H, W, dtype)
        out[n] = bilinear(frames[n], sx, sy, dtype)
    if frames.dtype == np.uint8 and not raw:
        return np.clip(np.rint(out), 0, 255).astype(np.uint8)
    return out


# ----------------------------------------------------------------------------- outline
def outline(R, H, W, hw, hfov_deg, border_px=3, dtype=np.float64):
    """One camera R [3, 3] on the H x W panorama -> (mask bool [H, W], u, v, d_f [H, W] in dtype, thresholds (tx, ty, tx - b,
    ty - b) in dtype).  A non-finite R has an empty mask."""
    tx, ty = view_tangents(hw, hfov_deg, dtype)
    b = dtype(float(border_px) * 2.0 * np.tan(0.5 * np.deg2rad(float(hfov_deg))) / hw[1])
    px, py, pz = _pixel_dirs(H, W, dtype)
    Rd = np.asarray(R, np.float64).astype(dtype)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        df = Rd[0, 0] * px + Rd[1, 0] * py + Rd[2, 0] * pz
        du = Rd[0, 1] * px + Rd[1, 1] * py + Rd[2, 1] * pz
        dr = Rd[0, 2] * px + Rd[1, 2] * py + Rd[2, 2] * pz
        u, v = dr / df, du / df
        au, av = np.abs(u), np.abs(v)
        inside = (df > 0) & (au <= tx) & (av <= ty)
        inner = (au <= tx - b) & (av <= ty - b)
    mask = inside & ~inner
    if not np.all(np.isfinite(Rd)):
        mask = np.zeros((H, W), bool)
    return mask, u, v, df, (tx, ty, tx - b, ty - b)


def draw(frames, masks, rgb):
    """frames u8 [N, H, W, 3] with rgb at the masks' pixels."""
    out = np.array(frames, copy=True)
    out[np.asarray(masks)] = np.asarray(rgb, np.uint8)
    return out


# ----------------------------------------------------------------------------- smooth and peak
def _map_terms(hm, wm, sigma_deg, dtype):
    px, py, pz = (a.reshape(-1) for a in _pixel_dirs(hm, wm, dtype))
    a = np.repeat(tables(hm, wm, dtype)[2], wm)
    sigma = np.deg2rad(float(sigma_deg))
    return px, py, pz, a, dtype(1.0 / (sigma * sigma))


def _clean(s, dtype):
    s = np.asarray(s).astype(dtype).reshape(-1)
    return np.where(np.isfinite(s), s, dtype(0))


def smooth(maps, sigma_deg=15.0, dtype=np.float64):
    """maps [F, hm, wm] -> float64 [F, hm, wm] (the quotient of the two float64 sums, not rounded); non-finite values count 0."""
    maps = np.asarray(maps)
    F, hm, wm = maps.shape
    px, py, pz, a, kappa = _map_terms(hm, wm, sigma_deg, dtype)
    dot = px[:, None] * px[None, :] + py[:, None] * py[None, :] + pz[:, None] * pz[None, :]
    e = np.exp(kappa * (dot - dtype(1)))
    den = np.sum((a[None, :] * e).astype(np.float64), 1)
    out = np.empty((F, hm, wm))
    for f in range(F):
        a_s = a * _clean(maps[f], dtype)
        out[f] = (np.sum((a_s[None, :] * e).astype(np.float64), 1) / den).reshape(hm, wm)
    return out


def argmax_finite(v):
    """The lowest index of the largest finite value of v (flattened); -1 when nothing is finite."""
    v = np.asarray(v).reshape(-1)
    fin = np.isfinite(v)
    if not fin.any():
        return -1
    return int(np.argmax(np.where(fin, v, -np.inf)))


def peak(maps, sigma_deg=15.0, dtype=np.float64, smoothed=None):
    """maps [F, hm, wm] -> (dirs float64 [F, 3], idx int [F], val [F]).  `smoothed` defaults to smooth(maps, sigma_deg, dtype),
    which float32 rounds once as the device's buffer does."""
    maps = np.asarray(maps)
    F, hm, wm = maps.shape
    sm = smooth(maps, sigma_deg, dtype) if smoothed is None else np.asarray(smoothed)
    sm = sm.astype(dtype)
    px, py, pz, a, kappa = _map_terms(hm, wm, sigma_deg, dtype)
    dirs, idx, val = np.empty((F, 3)), np.empty(F, np.int64), np.empty(F)
    for f in range(F):
        k = argmax_finite(sm[f])
        if k < 0 or not np.isfinite(np.asarray(maps[f], np.float64)).any():
            dirs[f], idx[f], val[f] = (1.0, 0.0, 0.0), -1, np.nan
            continue
        dot = px[k] * px + py[k] * py + pz[k] * pz
        e = np.exp(kappa * (dot - dtype(1)))
        wgt = (a * _clean(maps[f], dtype)) * e
        c = np.array([np.sum((wgt * q).astype(np.float64)) for q in (px, py, pz)])
        n = float(np.linalg.norm(c))
        dirs[f] = c / n if n > 0.0 and np.isfinite(n) else (px[k], py[k], pz[k])
        idx[f], val[f] = k, sm[f].reshape(-1)[k]
    return dirs, idx, val


def map_position(d, hm, wm):
    """The real-valued map position (x, y) of the direction d, float64."""
    sx, sy = pix(np.asarray(d, np.float64), hm, wm)
    return float(sx), float(sy)


# ----------------------------------------------------------------------------- the camera path (host code of utils/viewport.py)
def look_at(c, prev_right=None):
    """Columns (f, up, right): right = normalize(f x (0, 1, 0)), up = right x f; at a pole (|f x y| < 1e-6) prev_right, or
    (0, 0, 1), made perpendicular to f."""
    f = np.asarray(c, np.float64)
    f = f / np.sqrt(f @ f)
    r = np.array([-f[2], 0.0, f[0]])                                  # f x (0, 1, 0)
    if np.sqrt(r @ r) < 1e-6:
        r = np.array([0.0, 0.0, 1.0]) if prev_right is None else np.asarray(prev_right, np.float64)
        r = r - (r @ f) * f
    r = r / np.sqrt(r @ r)
    up = np.array([r[1] * f[2] - r[2] * f[1], r[2] * f[0] - r[0] * f[2], r[0] * f[1] - r[1] * f[0]])
    return np.stack([f, up, r], 1)


def _step_towards(m, c, fraction, max_step):
    cr = np.cross(m, c)
    s, d = float(np.sqrt(cr @ cr)), float(m @ c)
    step = fraction * np.arctan2(s, d)
    if max_step is not None and step > max_step:
        step = max_step
    if s < 1e-12:
        if d > 0.0:
            return m
        y = np.array([0.0, 1.0, 0.0])
        cy = np.cross(m, y)
        a = y if np.sqrt(cy @ cy) >= 1e-6 else np.array([0.0, 0.0, 1.0])
        a = a - (a @ m) * m
        a = a / np.sqrt(a @ a)
    else:
        a = cr / s
    p = m * np.cos(step) + np.cross(a, m) * np.sin(step)
    return p / np.sqrt(p @ p)


def smooth_path(c, alpha=0.85, max_step_deg=None):
    """Forward: m_0 = c_0, m_t = from m_t-1 towards c_t at the fraction 1 - alpha of the angle, at most max_step_deg; then the
    same pass backwards over the result; re-normalised."""
    c = np.asarray(c, np.float64)
    c = c / np.sqrt(np.sum(c * c, 1))[:, None]
    max_step = None if max_step_deg is None else np.deg2rad(float(max_step_deg))

    def run(seq):
        out = [seq[0]]
        for t in range(1, len(seq)):
            out.append(_step_towards(out[-1], seq[t], 1.0 - alpha, max_step))
        return np.stack(out)

    out = run(run(c)[::-1])[::-1]
    return out / np.sqrt(np.sum(out * out, 1))[:, None]


def cameras(path):
    """look_at of every direction with the previous frame's right chained: [F, 3, 3]."""
    out, right = [], None
    for p in np.asarray(path, np.float64):
        R = look_at(p, right)
        right = R[:, 2]
        out.append(R)
    return np.stack(out)


def angle(a, b):
    """The angle between two directions in radians (atan2 of cross and dot: accurate for small angles)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.arctan2(np.linalg.norm(np.cross(a, b)), a @ b))


# ----------------------------------------------------------------------------- test inputs shared by the CPU and GPU tests
def vmf_blob(centre, hm, wm, sigma_deg):
    """exp(kappa (p . centre - 1)) on the hm x wm map, float64."""
    px, py, pz = _pixel_dirs(hm, wm, np.float64)
    c = np.asarray(centre, np.float64)
    c = c / np.linalg.norm(c)
    sigma = np.deg2rad(sigma_deg)
    return np.exp(((px * c[0] + py * c[1] + pz * c[2]) - 1.0) / (sigma * sigma))
