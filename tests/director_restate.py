"""Numpy restatement of the director (K20, csrc/viewport.hip and utils/viewport.py; the specification is DESIGN.md "K20"): several
cameras planned one after the other, each on the maps with the caps about the cameras before it taken out, and what the host does
with them.  The path, the refine step and the videos are tests/campath_restate.py's, geometry, smoothing and the path filter
tests/viewport_restate.py's, by import.

    exclude   out[t][j] = +0 where ((p_x d_x + p_y d_y) + p_z d_z) >= c in float32 for any direction d of frame t, c = cos(radius)
              rounded to float32 once, p the pixel centre from the float32 tables; else the input's bits.  A direction with a
              non-finite component excludes nothing
    plan      sm = smooth(maps) rounded to float32, g[t] = 4096 / max sm[t] in float32.  Camera 0: path(sm, g), refine(maps, idx).
              Camera k >= 1: D_k = the refined directions of cameras 0 .. k - 1 in float32; path(exclude(sm, D_k), g),
              refine(exclude(maps, D_k), idx_k).  One gain for all cameras: their scores compare
    share     score[k][s] / score[0][s], 0 where score[0][s] is 0; camera k >= 1 is dropped in the shots where it is below min_share
    arrange   'longitude': per shot the active cameras by wrap(lon(m_k) - lon(c)) into (-180, 180], m_k the normalised mean of the
              camera's filtered path over the shot, c the normalised sum of the m_k, lon = atan2(z, x); ties by index; dropped
              cameras last; where hypot(c_x, c_z) < 1e-9 the order stays
    best      per viewer the largest finite iou over the cameras that are finite in its frame, the lowest camera on ties

Nothing here imports the code under test.
"""
import numpy as np

from tests import campath_restate as cr
from tests import viewport_restate as vr
from tests.stabilize_restate import _pixel_dirs


# ----------------------------------------------------------------------------- exclusion
def cap_cos(radius_deg):
    """cos(radius) in float64, rounded to float32 once."""
    return np.float32(np.cos(np.deg2rad(float(radius_deg))))


def cap_dots(hm, wm, dirs, dtype=np.float32):
    """dirs [F, Kx, 3] -> the dot of every pixel centre with every direction, [F, Kx, hm wm], term by term in dtype."""
    px, py, pz = (a.reshape(-1).astype(dtype) for a in _pixel_dirs(hm, wm, dtype))
    d = np.asarray(dirs).astype(dtype)
    with np.errstate(invalid='ignore', over='ignore'):
        return (px * d[..., 0:1] + py * d[..., 1:2]) + pz * d[..., 2:3]


def usable(dirs):
    """dirs [F, Kx, 3] -> bool [F, Kx]: the directions whose components are all finite."""
    return np.isfinite(np.asarray(dirs, np.float64)).all(axis=-1)


def excluded(hm, wm, dirs, radius_deg):
    """dirs [F, Kx, 3] -> bool [F, hm wm]: the pixels inside any cap, as float32 decides it."""
    with np.errstate(invalid='ignore'):
        hit = (cap_dots(hm, wm, dirs) >= cap_cos(radius_deg)) & usable(dirs)[..., None]
    return hit.any(axis=1)


def exclude(maps, dirs, radius_deg):
    """maps [F, hm, wm] float32 -> a copy with the caps' pixels +0; every other pixel keeps its bits."""
    maps = np.asarray(maps, np.float32)
    F, hm, wm = maps.shape
    out = maps.copy()
    out.reshape(F, -1)[excluded(hm, wm, dirs, radius_deg)] = np.float32(0)
    return out


def cap_margin(hm, wm, dirs, radius_deg):
    """How far, in float64, the nearest pixel's dot with a usable direction is from the float32 threshold: where this exceeds
    what float32 can move a unit dot product, float32 and float64 take the same decision for every pixel."""
    ok = usable(dirs)
    if not ok.any():
        return np.inf
    dots = cap_dots(hm, wm, np.where(ok[..., None], np.asarray(dirs, np.float64), 0.0), np.float64)
    return float(np.abs(dots - np.float64(cap_cos(radius_deg)))[ok].min())


# ----------------------------------------------------------------------------- the plan
def plan_inputs(maps, sigma_deg=15.0):
    """(sm float32 [F, hm, wm], gain float32 [F]) as cr.plan_chain forms them."""
    maps = np.asarray(maps)
    F = maps.shape[0]
    sm = vr.smooth(maps, sigma_deg).astype(np.float32)
    val = np.array([sm[f].reshape(-1)[k] if k >= 0 else np.nan for f, k in ((f, vr.argmax_finite(sm[f])) for f in range(F))],
                   np.float32)
    with np.errstate(divide='ignore', invalid='ignore'):
        return sm, np.float32(cr.VOTE_MAX) / val


def plan_multi(maps, n, exclude_deg=45.0, sigma_deg=15.0, cuts=None, turn_cost=16.0, step_deg=15.0, inputs=None, before=None):
    """maps [F, hm, wm] -> (idx int64 [n, F], score int64 [n, S], fine float64 [n, F, 3], margin).  ``inputs``: (sm, gain) other
    than plan_inputs(maps)'s; ``before`` float32 [n, F, 3]: the refined directions the caps are drawn about, instead of this
    function's own rounded to float32 - a test of the device hands in the device's, so that every camera is judged on the same
    caps.  margin: the smallest cap_margin of any cap drawn."""
    maps = np.asarray(maps, np.float32)
    F, hm, wm = maps.shape
    sm, gain = plan_inputs(maps, sigma_deg) if inputs is None else inputs
    starts = [lo for lo, _ in cr.segments(cuts, F)] + [F]
    idx, score, fine, margin = [], [], [], np.inf
    for k in range(n):
        sm_k, raw_k = sm, maps
        if k >= 1:
            D = (np.stack(fine).astype(np.float32) if before is None else np.asarray(before, np.float32)[:k]).transpose(1, 0, 2)
            margin = min(margin, cap_margin(hm, wm, D, exclude_deg))
            sm_k, raw_k = exclude(sm, D, exclude_deg), exclude(maps, D, exclude_deg)
        i, s = cr.path(sm_k, gain, turn_cost, step_deg, starts)
        idx.append(i)
        score.append(s)
        fine.append(cr.refine(raw_k, i, sigma_deg))
    return np.stack(idx), np.stack(score), np.stack(fine), margin


# ----------------------------------------------------------------------------- the host half
def longitude_order(means):
    means = np.asarray(means, np.float64)
    c = means.sum(axis=0)
    if np.hypot(c[0], c[2]) < 1e-9:
        return list(range(len(means)))
    lon_c = np.rad2deg(np.arctan2(c[2], c[0]))
    keys = []
    for m in means:
        d = np.rad2deg(np.arctan2(m[2], m[0])) - lon_c
        while d <= -180.0:
            d += 360.0
        while d > 180.0:
            d -= 360.0
        keys.append(d)
    return sorted(range(len(means)), key=lambda k: (keys[k], k))


def multi_cameras(dirs, score, cuts=None, alpha=0.85, min_share=0.0, arrange='score'):
    """dirs [n, F, 3], score [n, S] -> (R float64 [F, n, 3, 3], NaN where a camera is dropped; share float64 [n, S]), both by
    position: 'score' keeps every camera's place, 'longitude' orders each shot's active cameras and puts the dropped ones last."""
    dirs, score = np.asarray(dirs, np.float64), np.asarray(score, np.float64)
    n, F = dirs.shape[:2]
    shots = cr.segments(cuts, F)
    paths = np.stack([cr.smooth_path(dirs[k], alpha, cuts) for k in range(n)])
    cams = np.stack([np.concatenate([vr.cameras(paths[k, lo:hi]) for lo, hi in shots]) for k in range(n)])
    share = np.array([[score[k][s] / score[0][s] if score[0][s] != 0 else 0.0 for s in range(len(shots))] for k in range(n)])
    R, placed = np.full((F, n, 3, 3), np.nan), np.zeros_like(share)
    for s, (lo, hi) in enumerate(shots):
        active = [k for k in range(n) if k == 0 or share[k][s] >= min_share]
        order = list(range(n))
        if arrange == 'longitude':
            means = []
            for k in active:
                m = paths[k, lo:hi].mean(axis=0)
                means.append(m / np.sqrt(m @ m))
            order = [active[j] for j in longitude_order(means)] + [k for k in range(n) if k not in active]
        for slot, k in enumerate(order):
            placed[slot][s] = share[k][s]
            if k in active:
                R[lo:hi, slot] = cams[k, lo:hi]
    return R, placed


def split_layout(n, hw, gutter=8, direction='row'):
    h, w = hw
    if direction == 'row':
        return [(k * (w + gutter), 0, w, h) for k in range(n)], (h, n * w + (n - 1) * gutter)
    return [(0, k * (h + gutter), w, h) for k in range(n)], (n * h + (n - 1) * gutter, w)


def canvas(views, tiles, canvas_hw, fill, dropped=()):
    """views: K arrays [N, h_k, w_k, C] -> the canvas [N, hc, wc, C]: fill, then every tile's view; ``dropped``: the tiles that
    stay fill."""
    N, C = views[0].shape[0], views[0].shape[3]
    out = np.empty((N, canvas_hw[0], canvas_hw[1], C), views[0].dtype)
    out[:] = np.asarray(fill, views[0].dtype)
    for k, (x0, y0, w, h) in enumerate(tiles):
        if k not in dropped:
            out[:, y0:y0 + h, x0:x0 + w] = views[k]
    return out


# ----------------------------------------------------------------------------- the best of n cameras per viewer
def best_of(iou, cam_finite, viewer_finite, frame, F):
    """iou float64 [n, N], cam_finite bool [n, N] (the camera is finite in the viewer's frame), viewer_finite bool [N], frame
    int [N] -> (best_iou [N], best_cam [N], frame_iou [F], the video's iou: the mean of the frames that have one)."""
    n, N = iou.shape
    best_iou, best_cam = np.full(N, np.nan), np.full(N, -1, np.int64)
    for v in range(N):
        for k in range(n):
            if cam_finite[k][v] and np.isfinite(iou[k][v]) and (best_cam[v] < 0 or iou[k][v] > best_iou[v]):
                best_iou[v], best_cam[v] = iou[k][v], k
    frame_iou = np.full(F, np.nan)
    for f in range(F):
        mine = [v for v in range(N) if frame[v] == f and viewer_finite[v]]
        if mine:
            frame_iou[f] = sum(best_iou[v] for v in mine) / len(mine)
    has = ~np.isnan(frame_iou)
    return best_iou, best_cam, frame_iou, float(frame_iou[has].mean()) if has.any() else float('nan')
