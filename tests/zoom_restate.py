"""Float64 numpy restatement of zoom (K22, csrc/viewport.hip: view_spread_kernel and the lens; utils/viewport.py: spread_constant,
zoom_from_spread, smooth_zoom; the specification is DESIGN.md "K22").  The views, outlines and agreements under a lens are K12's,
K21's and K17's with that frame's field of view: tests/viewport_restate.py, viewport_aa_restate.py and headtrack_restate.py.

    lens     (tx, ty, b, 0) = (tan(hfov / 2), tan(hfov / 2) h / w, border_px 2 tan(hfov / 2) / w, 0): float64 values rounded once
    spread   d = dirs[f]; in_j = ((p_x d_x + p_y d_y) + p_z d_z) >= cos(window); top = the largest finite s_j in the cap;
             m_j = a_j max(s_j - level top, 0) for the finite s_j in the cap, else 0; g_j = ((p_x - d_x)^2 + (p_y - d_y)^2 + (p_z -
             d_z)^2) / 2; q = sum m_j g_j / sum m_j.  NaN for a non-finite d, a cap without a finite pixel, top <= 0, or a sum of
             m that is not positive and finite
    c(level) the q of a narrow Gaussian blob of width 1: (1 - (1 + L) level - level L^2 / 2) / (1 - level - level L), L = -ln level
    zoom     sigma_b = sqrt(q / c), tx = tan(min(sigmas sigma_b, radians(89))) max(1, w / h), hfov = 2 atan(tx) clamped; NaN: default
    smooth   z = log(tan(hfov / 2)); a pass is m_0 = z_0, m_t = m_t-1 + (1 - alpha) (z_t - m_t-1); the mean of forward-then-backward
             and backward-then-forward, shot by shot

``dtype=np.float32`` evaluates every per-pixel term in float32, operation by operation as the kernel does, and keeps the sums in
float64: d32 = |spread(float32) - spread(float64)| is the unit of the GPU tests' bounds, as for K11.  Nothing here imports the
code under test.
"""
import numpy as np

from tests import viewport_restate as vr
from tests.stabilize_restate import _pixel_dirs, tables


# ----------------------------------------------------------------------------- the lens
def lens(hfov_deg, hw, border_px=0.0, dtype=np.float32):
    """[N, 4] = (tx, ty, b, 0): K12a's tangents (``viewport_restate.view_tangents``) and K12b's b (``viewport_restate.outline``'s
    expression), float64 values rounded once to dtype."""
    fov = np.atleast_1d(np.asarray(hfov_deg, np.float64))
    out = np.zeros((len(fov), 4), dtype)
    for n, v in enumerate(fov):
        out[n, 0], out[n, 1] = vr.view_tangents(hw, v, dtype)
        out[n, 2] = dtype(float(border_px) * 2.0 * np.tan(0.5 * np.deg2rad(float(v))) / hw[1]) if border_px != 0 else dtype(0)
    return out


# ----------------------------------------------------------------------------- spread
def cap_dots(d, hm, wm, dtype=np.float64):
    """The dot product of every pixel centre with the direction d (its float32 value), in the kernel's order: [hm wm] in dtype."""
    px, py, pz = (a.reshape(-1) for a in _pixel_dirs(hm, wm, dtype))
    d = np.asarray(d, np.float32).astype(dtype)
    return (px * d[0] + py * d[1]) + pz * d[2]


def cap_margin(d, hm, wm, window_deg):
    """(the smallest |dot - cos(window)| over the pixels in float64, d32 = the largest float32-to-float64 difference of a dot
    product or of the threshold): a cap whose margin exceeds 8 d32 holds the same pixels in float32 and in float64."""
    d64, d32 = cap_dots(d, hm, wm), cap_dots(d, hm, wm, np.float32)
    cw = np.cos(np.deg2rad(float(window_deg)))
    err = max(float(np.max(np.abs(d32.astype(np.float64) - d64))), abs(float(np.float32(cw)) - cw))
    return float(np.min(np.abs(d64 - cw))), err


def spread(maps, dirs, window_deg=45.0, level=0.5, dtype=np.float64, check_margin=False):
    """maps [F, hm, wm], dirs [F, 3] (as the device holds them: float32 values) -> q float64 [F] (the quotient of the two float64
    sums, not rounded).  check_margin: assert that no pixel's dot product lies within 8 d32 of cos(window) for a finite d."""
    maps, dirs = np.asarray(maps), np.asarray(dirs, np.float32)
    F, hm, wm = maps.shape
    px, py, pz = (a.reshape(-1) for a in _pixel_dirs(hm, wm, dtype))
    a = np.repeat(tables(hm, wm, dtype)[2], wm)
    cw, lv, half = dtype(np.cos(np.deg2rad(float(window_deg)))), dtype(level), dtype(0.5)
    q = np.full(F, np.nan)
    for f in range(F):
        if not np.all(np.isfinite(dirs[f])):
            continue
        if check_margin:
            margin, d32 = cap_margin(dirs[f], hm, wm, window_deg)
            assert margin > 8 * d32, (f, margin, d32)
        d = dirs[f].astype(dtype)
        s = maps[f].reshape(-1).astype(dtype)
        take = (cap_dots(dirs[f], hm, wm, dtype) >= cw) & np.isfinite(s)
        if not take.any():
            continue
        top = np.max(s[take])
        if not top > 0:
            continue
        m = np.where(take, a * np.maximum(np.where(take, s, dtype(0)) - lv * top, dtype(0)), dtype(0))
        ex, ey, ez = px - d[0], py - d[1], pz - d[2]
        g = half * ((ex * ex + ey * ey) + ez * ez)
        M, Q = float(np.sum(m.astype(np.float64))), float(np.sum((m * g).astype(np.float64)))
        if M > 0.0 and np.isfinite(M):
            q[f] = Q / M
    return q


def spread_constant(level=0.5):
    L = -np.log(float(level))
    return float((1.0 - (1.0 + L) * level - 0.5 * level * L * L) / (1.0 - level - level * L))


def spread_constant_numeric(level=0.5, n=200001):
    """c(level) by numerical integration: for the planar blob exp(-r^2 / 2) the mean of r^2 / 2 weighted by (blob - level) r dr
    over the disc where the blob stands above level (Simpson's rule on n points)."""
    r1 = np.sqrt(-2.0 * np.log(float(level)))
    r = np.linspace(0.0, r1, n)
    w = np.ones(n)
    w[1:-1:2], w[2:-1:2] = 4.0, 2.0
    excess = (np.exp(-0.5 * r * r) - level) * r
    return float(np.sum(w * excess * 0.5 * r * r) / np.sum(w * excess))


# ----------------------------------------------------------------------------- the host chain
def zoom_from_spread(q, hw, level=0.5, sigmas=2.5, range_deg=(40.0, 110.0), default_deg=90.0):
    h, w = hw
    out = []
    for v in np.atleast_1d(np.asarray(q, np.float64)):
        if np.isnan(v):
            out.append(float(default_deg))
            continue
        sigma_b = np.sqrt(v / spread_constant(level))
        tx = np.tan(min(sigmas * sigma_b, np.deg2rad(89.0))) * max(1.0, w / h)
        out.append(float(min(max(np.rad2deg(2.0 * np.arctan(tx)), range_deg[0]), range_deg[1])))
    return np.array(out)


def _pass(z, alpha):
    out = [z[0]]
    for t in range(1, len(z)):
        out.append(out[-1] + (1.0 - alpha) * (z[t] - out[-1]))
    return np.array(out)


def smooth_zoom(hfov_deg, alpha=0.9, cuts=None):
    x = np.asarray(hfov_deg, np.float64)
    edges = [0] + sorted(cuts or []) + [len(x)]
    out = []
    for lo, hi in zip(edges[:-1], edges[1:]):
        z = np.log(np.tan(0.5 * np.deg2rad(x[lo:hi])))
        fb = _pass(_pass(z, alpha)[::-1], alpha)[::-1]
        bf = _pass(_pass(z[::-1], alpha)[::-1], alpha)
        out.append(np.rad2deg(2.0 * np.arctan(np.exp(0.5 * (fb + bf)))))
    return np.concatenate(out)


def track(dirs, q, hw, hfov_deg=90.0, alpha=0.85, max_step_deg=None, zoom=True, level=0.5, sigmas=2.5, range_deg=(40.0, 110.0),
          zoom_alpha=0.9):
    """The host half of ``ViewportPilot.track`` without cuts: dirs [F, 3] and q [F] as they come from the device -> (R float64
    [F, 3, 3], hfov_deg float64 [F])."""
    R = vr.cameras(vr.smooth_path(dirs, alpha, max_step_deg))
    if not zoom:
        return R, np.full(len(R), float(hfov_deg))
    return R, smooth_zoom(zoom_from_spread(q, hw, level, sigmas, range_deg, hfov_deg), zoom_alpha)


# ----------------------------------------------------------------------------- test inputs shared by the CPU and GPU tests
def gaussian_blob(centre, hm, wm, sigma_deg):
    """exp(-theta^2 / (2 sigma^2)) of the angle theta to `centre` on the hm x wm map, float64."""
    px, py, pz = _pixel_dirs(hm, wm, np.float64)
    c = np.asarray(centre, np.float64)
    c = c / np.linalg.norm(c)
    cr = np.stack([py * c[2] - pz * c[1], pz * c[0] - px * c[2], px * c[1] - py * c[0]])
    theta = np.arctan2(np.sqrt(np.sum(cr * cr, 0)), px * c[0] + py * c[1] + pz * c[2])
    sigma = np.deg2rad(float(sigma_deg))
    return np.exp(-0.5 * (theta / sigma) ** 2)


def direction(lon_deg, lat_deg):
    lon, lat = np.deg2rad(float(lon_deg)), np.deg2rad(float(lat_deg))
    return np.array([np.cos(lat) * np.cos(lon), np.sin(lat), np.cos(lat) * np.sin(lon)])


def scene(seed, hm, wm, centre, sigma_deg, noise=0.1, second=True):
    """A blob of height 1 and width sigma_deg at `centre`, uniform noise of `noise` of its height, and a second blob of the same
    height and width 90 degrees away (about the axis perpendicular to the centre and (0, 1, 0), or (0, 0, 1) at a pole)."""
    from tests.stabilize_restate import rot
    c = np.asarray(centre, np.float64) / np.linalg.norm(centre)
    s = gaussian_blob(c, hm, wm, sigma_deg)
    if second:
        axis = np.cross(c, (0.0, 1.0, 0.0))
        axis = axis if np.linalg.norm(axis) > 1e-6 else np.array([0.0, 0.0, 1.0])
        s = np.maximum(s, gaussian_blob(rot(axis, 0.5 * np.pi) @ c, hm, wm, sigma_deg))
    return s + noise * np.random.default_rng(seed).random((hm, wm))
