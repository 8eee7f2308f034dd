"""The viewport pilot (K12, csrc/viewport.hip): what a 360-degree saliency map is used for - choosing where to look and rendering
that normal-field-of-view window.  The reference's ``utils/fov_visual.py`` (``box_proh``, ``fov_module``, ``draw_cube_fov_box``)
has this purpose and does not compile; the definition is the package's own (DESIGN.md "K12").

Per frame the saliency map is smoothed on the sphere and its peak refined by one mean-shift step (``ops.sphere_peak``); the peaks
become a smooth camera path on the host (``smooth_path``: a zero-phase exponential filter along great circles; ``look_at``: the
camera with a level horizon), and the views are rendered at the frames' own resolution (``ops.viewport_render``);
``ops.viewport_outline`` draws the view's frame on the panorama.  ``planner='viterbi'`` replaces the per-frame peaks by the path
that collects the most saliency under a turn limit and a turn cost (K16: ``ops.sphere_path``, then ``ops.sphere_refine``): it
chooses which of several targets to follow, where the peaks hop between them.  Several cameras at once (K20, DESIGN.md "K20"):
``plan_multi`` plans them one after the other, each on the maps with a cap about the cameras before it taken out
(``ops.sphere_exclude``), ``paths`` turns the plans into cameras, drops those that found nothing and orders them, and
``render_multi`` shows their views side by side on one canvas (``ops.viewport_render_multi``).  A camera is a rotation R,
camera-to-world, with the columns (forward, up, right): R = I looks at the panorama's centre.  A view coarser than its source is
anti-aliased by supersampling (K21, DESIGN.md "K21"): ``supersample_for`` is the factor a view needs, ``ViewportPilot(..,
antialias=True)`` uses it.  Zoom (K22, DESIGN.md "K22"): ``ops.sphere_spread`` measures how wide the target is,
``zoom_from_spread`` and ``smooth_zoom`` turn that into a field of view per frame, ``ViewportPilot(.., zoom=True).follow_zoom``
renders every frame through its own lens in one launch (``ops.viewport_render_zoom``).  Roll and translation are out of scope.
"""
import numpy as np
import torch

from .. import ops
from ._device import TabWork, host_tensor, on_device
from .shots import check_cuts, segments

_Y = np.array([0.0, 1.0, 0.0])
_Z = np.array([0.0, 0.0, 1.0])


def _unit(v):
    return v / np.linalg.norm(v)


def look_at(c, prev_right=None):
    """The camera that looks along the direction c with a level horizon: float64 [3, 3] with the columns (f, up, right),
    right = normalize(f x (0, 1, 0)), up = right x f.  At a pole (|f x y| < 1e-6) the horizon is undefined: ``prev_right`` (the
    previous frame's right, (0, 0, 1) for a first frame) is used, made perpendicular to f."""
    f = _unit(np.asarray(c, np.float64))
    r = np.cross(f, _Y)
    if np.linalg.norm(r) < 1e-6:
        r = _Z if prev_right is None else np.asarray(prev_right, np.float64)
        r = r - (r @ f) * f
    r = _unit(r)
    return np.stack([f, np.cross(r, f), r], axis=1)


def _towards(m, c, fraction, max_step):
    """The point on the great circle from m towards c at `fraction` of their angle, at most max_step radians away from m."""
    cr = np.cross(m, c)
    s, d = float(np.linalg.norm(cr)), float(m @ c)
    step = fraction * np.arctan2(s, d)
    if max_step is not None:
        step = min(step, max_step)
    if s < 1e-12:
        if d > 0.0:
            return m
        # antipodal: the great circle is undefined - turn about (0, 1, 0), about (0, 0, 1) when m is parallel to that
        a = _Y if np.linalg.norm(np.cross(m, _Y)) >= 1e-6 else _Z
        a = _unit(a - (a @ m) * m)
    else:
        a = cr / s
    return _unit(m * np.cos(step) + np.cross(a, m) * np.sin(step))


def _one_pass(c, alpha, max_step):
    out = np.empty_like(c)
    out[0] = c[0]
    for t in range(1, c.shape[0]):
        out[t] = _towards(out[t - 1], c[t], 1.0 - alpha, max_step)
    return out


def smooth_path(c, alpha=0.85, max_step_deg=None, cuts=None):
    """c [F, 3] unit directions -> float64 [F, 3]: m_0 = c_0, m_t = the point on the great circle from m_t-1 towards c_t at
    the fraction 1 - alpha of their angle (at most max_step_deg degrees), then the same pass backwards over the result (zero
    phase); re-normalised.  ``cuts`` (``utils.shots``: the first frame of every new shot): both passes run shot by shot, so the
    camera neither leaves for the next scene's peak before a cut nor is still arriving after it."""
    c = np.asarray(c, np.float64)
    if c.ndim != 2 or c.shape[1] != 3 or c.shape[0] < 1:
        raise ValueError("c must be [F, 3], got %s" % (c.shape,))
    if not 0.0 <= float(alpha) < 1.0 or (max_step_deg is not None and not float(max_step_deg) > 0.0):
        raise ValueError("alpha must be in [0, 1) and max_step_deg positive, got %r, %r" % (alpha, max_step_deg))
    shots = segments(cuts, c.shape[0])
    if len(shots) > 1:
        return np.concatenate([smooth_path(c[lo:hi], alpha, max_step_deg) for lo, hi in shots])
    c = c / np.linalg.norm(c, axis=1, keepdims=True)
    max_step = None if max_step_deg is None else np.deg2rad(float(max_step_deg))
    fwd = _one_pass(c, float(alpha), max_step)
    out = _one_pass(fwd[::-1], float(alpha), max_step)[::-1]
    return out / np.linalg.norm(out, axis=1, keepdims=True)


def cameras(path, cuts=None):
    """path [F, 3] -> float64 [F, 3, 3]: ``look_at`` of every direction, each frame's right handed to the next one - within a
    shot: the first frame of every shot (``cuts``) starts without one."""
    path = np.asarray(path, np.float64)
    starts = set(check_cuts(cuts, path.shape[0]))
    out, right = [], None
    for t, p in enumerate(path):
        R = look_at(p, None if t in starts else right)
        right = R[:, 2]
        out.append(R)
    return np.stack(out)


def split_layout(n, hw, gutter=8, direction='row'):
    """n tiles of hw = (h, w) pixels side by side ('row') or stacked ('column') with ``gutter`` pixels between them ->
    (tiles [(x0, y0, w, h)] * n, canvas_hw): what ``ViewportPilot.render_multi`` takes."""
    n, h, w, gutter = int(n), int(hw[0]), int(hw[1]), int(gutter)
    if not 1 <= n <= 8 or h < 1 or w < 1 or gutter < 0 or direction not in ('row', 'column'):
        raise ValueError("a layout needs 1 <= n <= 8, h, w >= 1, gutter >= 0 and direction 'row' or 'column', got %r, %r, %r, %r"
                         % (n, hw, gutter, direction))
    if direction == 'row':
        return [(k * (w + gutter), 0, w, h) for k in range(n)], (h, n * w + (n - 1) * gutter)
    return [(0, k * (h + gutter), w, h) for k in range(n)], (n * h + (n - 1) * gutter, w)


def supersample_for(HW, hw, hfov_deg, limit=4):
    """The supersampling factor (K21, ``ops.viewport_render(.., supersample=)``) that a view of hw = (h, w) pixels and hfov_deg
    degrees of H x W frames needs: rho = tan(hfov / 2) max(W, 2 H) / (pi w) is the number of source pixels per view pixel at the
    view's centre (the edges of a gnomonic view are finer), and the factor is min(limit, max(1, ceil(rho - 1e-9))).  float64."""
    (H, W), (h, w), limit = (int(v) for v in HW), (int(v) for v in hw), int(limit)
    if min(H, W, h, w) < 1 or not 0.0 < float(hfov_deg) < 180.0 or not 1 <= limit <= 4:
        raise ValueError("sizes must be positive, 0 < hfov_deg < 180 and 1 <= limit <= 4, got %r, %r, %r, %r" % (HW, hw, hfov_deg, limit))
    rho = np.tan(0.5 * np.deg2rad(float(hfov_deg))) * max(W, 2 * H) / (np.pi * w)
    return int(min(limit, max(1, int(np.ceil(rho - 1e-9)))))


# ----------------------------------------------------------------------------- zoom (K22)
def spread_constant(level=0.5):
    """c(level) of ``ops.sphere_spread``: for a Gaussian blob exp(-theta^2 / (2 sigma_b^2)) that is narrow against the cap, q = c
    sigma_b^2 - the mean of theta^2 / 2 over the disc where the blob stands above ``level`` of its peak, weighted by its excess.
    With L = -ln(level): c = (1 - (1 + L) level - level L^2 / 2) / (1 - level - level L); c(0.5) = 0.21713."""
    level = float(level)
    if not 0.0 < level < 1.0:
        raise ValueError("level must be in (0, 1), got %r" % (level,))
    L = -np.log(level)
    return float((1.0 - (1.0 + L) * level - 0.5 * level * L * L) / (1.0 - level - level * L))


def zoom_from_spread(q, hw, level=0.5, sigmas=2.5, range_deg=(40.0, 110.0), default_deg=90.0):
    """q [F] (``ops.sphere_spread``) -> the field of view of every frame, float64 [F] in degrees: sigma_b = sqrt(q / c(level)) is
    the target's width, the shorter side of the view of hw = (h, w) pixels spans +- sigmas sigma_b (at most 89 degrees), so tx =
    tan(min(sigmas sigma_b, radians(89))) max(1, w / h) and hfov = 2 atan(tx), clamped to ``range_deg``.  A NaN q (no target)
    gives ``default_deg``.  2.5 widths and 40 .. 110 degrees are conventions, not tuned on data."""
    q = np.atleast_1d(np.asarray(q, np.float64))
    h, w = int(hw[0]), int(hw[1])
    lo, hi = float(range_deg[0]), float(range_deg[1])
    if q.ndim != 1 or h < 1 or w < 1 or not float(sigmas) > 0.0 or not 0.0 < lo <= hi < 180.0 or not 0.0 < float(default_deg) < 180.0:
        raise ValueError("q must be [F], hw positive, sigmas > 0, 0 < range_deg[0] <= range_deg[1] < 180 and 0 < default_deg < 180, "
                         "got %s, %r, %r, %r, %r" % (q.shape, hw, sigmas, range_deg, default_deg))
    with np.errstate(invalid='ignore'):
        sigma_b = np.sqrt(q / spread_constant(level))
        tx = np.tan(np.minimum(float(sigmas) * sigma_b, np.deg2rad(89.0))) * max(1.0, w / h)
        hfov = np.clip(np.rad2deg(2.0 * np.arctan(tx)), lo, hi)
    return np.where(np.isnan(q), float(default_deg), hfov)


def _scalar_pass(x, alpha):
    out = np.empty_like(x)
    out[0] = x[0]
    for t in range(1, x.shape[0]):
        out[t] = out[t - 1] + (1.0 - alpha) * (x[t] - out[t - 1])
    return out


def smooth_zoom(hfov_deg, alpha=0.9, cuts=None):
    """hfov_deg [F] in degrees -> float64 [F]: ``smooth_path``'s zero-phase exponential filter on z = log(tan(hfov / 2)) - zoom
    multiplies, so the filter works in that log domain -, shot by shot (``cuts``).  A pass is m_0 = z_0, m_t = m_t-1 + (1 - alpha)
    (z_t - m_t-1); the result is the mean of forward-then-backward and backward-then-forward, which a scalar can afford and a
    great circle cannot: the filter is then exactly symmetric under time reversal, edges included."""
    x = np.asarray(hfov_deg, np.float64)
    if x.ndim != 1 or x.shape[0] < 1 or not np.all((x > 0.0) & (x < 180.0)):
        raise ValueError("hfov_deg must be [F] with every value in (0, 180), got %s" % (x.shape,))
    if not 0.0 <= float(alpha) < 1.0:
        raise ValueError("alpha must be in [0, 1), got %r" % (alpha,))
    shots = segments(cuts, x.shape[0])
    if len(shots) > 1:
        return np.concatenate([smooth_zoom(x[lo:hi], alpha) for lo, hi in shots])
    z, alpha = np.log(np.tan(0.5 * np.deg2rad(x))), float(alpha)
    fb = _scalar_pass(_scalar_pass(z, alpha)[::-1], alpha)[::-1]
    bf = _scalar_pass(_scalar_pass(z[::-1], alpha)[::-1], alpha)
    return np.rad2deg(2.0 * np.arctan(np.exp(0.5 * (fb + bf))))


def _longitude_deg(v):
    return np.rad2deg(np.arctan2(v[2], v[0]))


def longitude_order(means):
    """means float64 [m, 3], the unit mean directions of a shot's active cameras -> their order from left to right on the
    panorama: by wrap(lon(m_k) - lon(c)) into (-180, 180] with c the normalised sum of the means and lon = atan2(z, x), ties by
    index.  Where c has no longitude (hypot(c_x, c_z) < 1e-9) the given order stays."""
    means = np.asarray(means, np.float64)
    c = means.sum(axis=0)
    if np.hypot(c[0], c[2]) < 1e-9:
        return list(range(len(means)))
    keys = [180.0 - ((180.0 - (_longitude_deg(m) - _longitude_deg(c))) % 360.0) for m in means]
    return sorted(range(len(means)), key=lambda k: (keys[k], k))


def multi_cameras(dirs, score, cuts=None, alpha=0.85, max_step_deg=None, min_share=0.0, arrange='score'):
    """The host half of ``ViewportPilot.paths``, float64: dirs [n, F, 3], the planned directions of n cameras, and score [n, S],
    their votes per shot -> (R [F, n, 3, 3], share [n, S]).  Every camera's path is ``smooth_path`` and ``cameras`` with
    ``cuts``; share[k][s] = score[k][s] / score[0][s] (0 where score[0][s] is 0).  Camera k >= 1 is dropped in the shots where
    its share is below min_share: its R is NaN there.  arrange 'score' keeps the cameras in their order; 'longitude' puts every
    shot's active cameras in ``longitude_order`` of the normalised means of their filtered paths over the shot, the dropped ones
    behind them - R and share are then both by position."""
    dirs, score = np.asarray(dirs, np.float64), np.asarray(score, np.float64)
    if dirs.ndim != 3 or dirs.shape[2] != 3 or not 1 <= dirs.shape[0] <= 8 or dirs.shape[1] < 1:
        raise ValueError("dirs must be [n, F, 3] with 1 <= n <= 8, got %s" % (dirs.shape,))
    if not 0.0 <= float(min_share) <= 1.0:
        raise ValueError("min_share must be in [0, 1], got %r" % (min_share,))
    if arrange not in ('score', 'longitude'):
        raise ValueError("arrange must be 'score' or 'longitude', got %r" % (arrange,))
    n, F = dirs.shape[:2]
    shots = segments(cuts, F)
    if score.shape != (n, len(shots)):
        raise ValueError("score must be [%d, %d], one value per camera and shot, got %s" % (n, len(shots), score.shape))
    paths = np.stack([smooth_path(dirs[k], alpha, max_step_deg, cuts) for k in range(n)])
    cams = np.stack([cameras(paths[k], cuts) for k in range(n)])
    with np.errstate(divide='ignore', invalid='ignore'):
        share = np.where(score[0] == 0, 0.0, score / score[0])
    R, placed = np.full((F, n, 3, 3), np.nan), np.zeros_like(share)
    for s, (lo, hi) in enumerate(shots):
        active = [k for k in range(n) if k == 0 or share[k][s] >= float(min_share)]
        order = list(range(n))
        if arrange == 'longitude':
            means = [_unit(paths[k, lo:hi].mean(axis=0)) for k in active]
            order = [active[j] for j in longitude_order(means)] + [k for k in range(n) if k not in active]
        for slot, k in enumerate(order):
            placed[slot][s] = share[k][s]
            if k in active:
                R[lo:hi, slot] = cams[k, lo:hi]
    return R, placed


class MultiAgreement:
    """What ``ViewportPilot.agreement_multi`` returns, on the device: ``best_iou`` float64 [N], the largest finite ``iou`` of the
    viewer over the cameras that are finite in its frame (NaN without any), ``best_cam`` int64 [N], that camera (the lowest on
    ties, -1 without any); ``frame_iou``, ``centre_angle_deg`` (of the best camera) and ``finite`` as ``HeadAgreement``'s, so
    that ``HeadMaps.means`` takes it; ``cameras``, the n ``HeadAgreement``s."""

    def __init__(self, best_iou, best_cam, frame_iou, centre_angle_deg, finite, cameras):
        self.best_iou, self.best_cam, self.frame_iou = best_iou, best_cam, frame_iou
        self.centre_angle_deg, self.finite, self.cameras = centre_angle_deg, finite, cameras


class ViewportPilot:
    """``ViewportPilot((h, w), hfov_deg)``: views of h x w pixels that follow the saliency maps' peak.  Holds the workspaces.

    ``planner``: 'peak', every frame's own peak, or 'viterbi', the best path of K16 under ``turn_cost`` (votes per degree turned;
    a frame's peak votes 4096) and ``plan_step_deg`` (the most the path may turn between two frames).  16 per degree and 15
    degrees are conventions, chosen on the synthetic videos of tests/campath_restate.py and not tuned on data.

    ``antialias`` (K21): False renders with one bilinear sample per view pixel; True supersamples every view by
    ``supersample_for`` of the frames it is given - in ``render_multi`` per tile; an int 1 .. 4 is that factor.  ``render``,
    ``follow``, ``render_multi`` and ``follow_multi`` honour it.

    ``zoom`` (K22): True lets ``track`` and ``follow_zoom`` choose a field of view per frame from how wide the target is
    (``ops.sphere_spread`` inside ``zoom_window_deg`` degrees of the path's direction, above ``zoom_level`` of the peak there;
    ``zoom_from_spread`` with ``zoom_sigmas`` and ``zoom_range_deg``; ``smooth_zoom`` with ``zoom_alpha``).  2.5 widths, 40 .. 110
    degrees, 45 degrees, 0.5 and 0.9 are conventions, not tuned on data.  ``render``, ``outline`` and ``agreement`` take the
    fields of view as ``hfov_deg=``; a canvas (``render_multi``) keeps one field of view per call."""

    def __init__(self, hw=(720, 1280), hfov_deg=90.0, sigma_deg=15.0, alpha=0.85, max_step_deg=None, device='cuda', planner='peak',
                 turn_cost=16.0, plan_step_deg=15.0, antialias=False, zoom=False, zoom_sigmas=2.5, zoom_range_deg=(40.0, 110.0),
                 zoom_window_deg=45.0, zoom_level=0.5, zoom_alpha=0.9):
        if not isinstance(antialias, bool) and not (isinstance(antialias, (int, np.integer)) and 1 <= antialias <= 4):
            raise ValueError("antialias must be False, True or an int 1 .. 4, got %r" % (antialias,))
        self.antialias = antialias if isinstance(antialias, bool) else int(antialias)
        self.hw = (int(hw[0]), int(hw[1]))
        if min(self.hw) < 1 or not 0.0 < float(hfov_deg) < 180.0 or not float(sigma_deg) > 0.0:
            raise ValueError("hw must be positive, 0 < hfov_deg < 180 and sigma_deg > 0, got %r, %r, %r" % (hw, hfov_deg, sigma_deg))
        if not 0.0 <= float(alpha) < 1.0 or (max_step_deg is not None and not float(max_step_deg) > 0.0):
            raise ValueError("alpha must be in [0, 1) and max_step_deg positive, got %r, %r" % (alpha, max_step_deg))
        self.hfov_deg, self.sigma_deg, self.alpha = float(hfov_deg), float(sigma_deg), float(alpha)
        self.max_step_deg = None if max_step_deg is None else float(max_step_deg)
        if planner not in ('peak', 'viterbi'):
            raise ValueError("planner must be 'peak' or 'viterbi', got %r" % (planner,))
        if not 0.0 <= float(turn_cost) <= 4096.0 or not 0.0 < float(plan_step_deg) <= 180.0:
            raise ValueError("turn_cost must be in [0, 4096] and plan_step_deg in (0, 180], got %r, %r" % (turn_cost, plan_step_deg))
        self.planner, self.turn_cost, self.plan_step_deg = planner, float(turn_cost), float(plan_step_deg)
        self.zoom, self.zoom_sigmas, self.zoom_window_deg = bool(zoom), float(zoom_sigmas), float(zoom_window_deg)
        self.zoom_range_deg = (float(zoom_range_deg[0]), float(zoom_range_deg[1]))
        self.zoom_level, self.zoom_alpha = float(zoom_level), float(zoom_alpha)
        if not self.zoom_sigmas > 0.0 or not 0.0 < self.zoom_range_deg[0] <= self.zoom_range_deg[1] < 180.0 \
                or not 0.0 < self.zoom_window_deg <= 180.0 or not 0.0 < self.zoom_level < 1.0 or not 0.0 <= self.zoom_alpha < 1.0:
            raise ValueError("zoom needs zoom_sigmas > 0, 0 < zoom_range_deg[0] <= zoom_range_deg[1] < 180, zoom_window_deg in "
                             "(0, 180], zoom_level in (0, 1) and zoom_alpha in [0, 1), got %r, %r, %r, %r, %r"
                             % (zoom_sigmas, zoom_range_deg, zoom_window_deg, zoom_level, zoom_alpha))
        self.device = torch.device(device)
        self._tab_work = TabWork()
        self._path_work = None

    def peaks(self, maps):
        """maps f32 [F, hm, wm] -> the direction of every map's peak, f32 [F, 3] on the device."""
        maps = on_device(maps, self.device, torch.float32)
        return ops.sphere_peak(maps, self.sigma_deg, work=self._tab_work(maps))[0]

    def plan(self, maps, cuts=None):
        """maps f32 [F, hm, wm] -> the directions of the planned path, f32 [F, 3] on the device: the maps smoothed, every frame's
        votes scaled so that its peak votes 4096, the best path over the map's pixels (``ops.sphere_path``; every shot of ``cuts``
        has its own) and one mean-shift step about each of its pixels (``ops.sphere_refine``).  No host synchronisation."""
        return self.plan_multi(maps, 1, cuts)[0][0]

    def plan_multi(self, maps, n, cuts=None, exclude_deg=None):
        """maps f32 [F, hm, wm] -> (dirs f32 [n, F, 3], score i32 [n, S]) on the device: the planned paths of n <= 8 cameras and
        the votes each collected in each of the S shots of ``cuts``.  Camera 0 is ``plan``'s.  Camera k >= 1 plans on the
        smoothed maps, and refines on the raw ones, with the caps of ``exclude_deg`` degrees about the refined directions of
        the cameras 0 .. k - 1 set to zero (``ops.sphere_exclude``): greedy, one target after the other.  Every camera votes
        with camera 0's gain, so the scores compare; camera k does not depend on n.  ``exclude_deg`` defaults to hfov_deg / 2:
        two targets closer than half a view fit in one view - a convention, not tuned on data.  Always the dynamic programme,
        whatever ``planner`` is.  No host synchronisation."""
        n = int(n)
        exclude_deg = 0.5 * self.hfov_deg if exclude_deg is None else float(exclude_deg)
        if not 1 <= n <= 8 or not 0.0 < exclude_deg <= 180.0:
            raise ValueError("n must be 1 .. 8 and exclude_deg in (0, 180], got %r, %r" % (n, exclude_deg))
        maps = host_tensor(maps)
        if maps.dim() != 3 or maps.numel() == 0:
            raise ValueError("maps must be a non-empty float32 [F, hm, wm], got %s" % (tuple(maps.shape),))
        F, hm = int(maps.shape[0]), int(maps.shape[1])
        if self.plan_step_deg < 180.0 / hm:
            raise ValueError("plan_step_deg %g is below the row pitch of a map of %d rows, %g degrees: no move is ever allowed"
                             % (self.plan_step_deg, hm, 180.0 / hm))
        edges = [0] + check_cuts(cuts, F) + [F]
        maps = on_device(maps, self.device, torch.float32)
        starts = torch.tensor(edges, dtype=torch.int32).to(self.device)
        work = self._tab_work(maps)
        sm = ops.sphere_smooth(maps, self.sigma_deg, work=work)
        val = ops.sphere_peak(maps, self.sigma_deg, smooth=sm, work=work)[2]
        gain = 4096.0 / val
        self._path_work = ops._work(ops.lib().cp360_path_work_bytes, "sphere_path", F, hm, int(maps.shape[2]), maps.device,
                                    self._path_work, " (F <= 65535, hm wm <= 16384)")
        dirs = torch.empty((n, F, 3), dtype=torch.float32, device=maps.device)
        score = torch.empty((n, len(edges) - 1), dtype=torch.int32, device=maps.device)
        sm_k, raw_k = sm, maps
        for k in range(n):
            if k == 1:
                sm_k, raw_k = torch.empty_like(sm), torch.empty_like(maps)
            if k >= 1:
                before = dirs[:k].permute(1, 0, 2).contiguous()
                ops.sphere_exclude(sm, before, exclude_deg, out=sm_k, work=work)
                ops.sphere_exclude(maps, before, exclude_deg, out=raw_k, work=work)
            idx, _, score[k] = ops.sphere_path(sm_k, gain, self.turn_cost, self.plan_step_deg, starts, work=self._path_work)
            dirs[k] = ops.sphere_refine(raw_k, idx, self.sigma_deg, work=work)
        return dirs, score

    def path(self, maps, cuts=None):
        """maps f32 [F, hm, wm] -> the cameras R f32 [F, 3, 3] on the device: the peaks (the planned path with the planner
        'viterbi'), copied to the host (3 F floats, the one synchronisation of a video), ``smooth_path`` and ``look_at`` with every
        frame's right chained, copied back.  With ``cuts`` (``utils.shots``) the path of every shot is its own: the concatenation
        of the shots' paths."""
        dirs = (self.plan(maps, cuts) if self.planner == 'viterbi' else self.peaks(maps)).cpu().numpy()
        R = cameras(smooth_path(dirs, self.alpha, self.max_step_deg, cuts), cuts)
        return torch.from_numpy(R.astype(np.float32)).to(self.device)

    def track(self, maps, cuts=None):
        """maps f32 [F, hm, wm] -> (R f32 [F, 3, 3] on the device, hfov_deg float64 [F] on the host): ``path``'s cameras and a
        field of view per frame.  The peaks (or the plan) exactly as ``path`` takes them, ``ops.sphere_spread`` about them on
        the device, ONE copy to the host of the 4 F floats (directions and spreads together: still the one synchronisation of a
        video), then ``smooth_path``, ``cameras``, ``zoom_from_spread`` and ``smooth_zoom``, all with ``cuts``.  With
        ``zoom=False`` R is ``path``'s bit for bit and hfov_deg is the pilot's constant."""
        maps = on_device(maps, self.device, torch.float32)
        dirs = self.plan(maps, cuts) if self.planner == 'viterbi' else self.peaks(maps)
        F = int(dirs.shape[0])
        if self.zoom:
            q = ops.sphere_spread(maps, dirs, self.zoom_window_deg, self.zoom_level, work=self._tab_work(maps))
            both = torch.cat([dirs.reshape(-1), q]).cpu().numpy()
            dirs, q = both[:3 * F].reshape(F, 3), both[3 * F:]
            hfov = smooth_zoom(zoom_from_spread(q, self.hw, self.zoom_level, self.zoom_sigmas, self.zoom_range_deg, self.hfov_deg),
                               self.zoom_alpha, cuts)
        else:
            dirs, hfov = dirs.cpu().numpy(), np.full(F, self.hfov_deg)
        R = cameras(smooth_path(dirs, self.alpha, self.max_step_deg, cuts), cuts)
        return torch.from_numpy(R.astype(np.float32)).to(self.device), hfov

    def _factor(self, frames, hw):
        """``antialias`` as the factor of a view of hw pixels of these frames."""
        if self.antialias is False:
            return 1
        if self.antialias is True:
            if frames.dim() != 4:
                raise ValueError("frames must be [N, H, W, C], got %s" % (tuple(frames.shape),))
            return supersample_for(frames.shape[1:3], hw, self.hfov_deg)
        return self.antialias

    @staticmethod
    def _fovs(hfov_deg, N):
        """``hfov_deg=`` of render / outline / agreement: N fields of view in degrees, float64 on the host."""
        fov = np.asarray(hfov_deg.cpu() if torch.is_tensor(hfov_deg) else hfov_deg, np.float64)
        if fov.shape != (N,) or not np.all((fov > 0.0) & (fov < 180.0)):
            raise ValueError("hfov_deg must be None or %d values in (0, 180), got %r" % (N, hfov_deg))
        return fov

    def render(self, frames, R, out=None, hfov_deg=None):
        """frames u8 [N, H, W, 3] or f32 [N, H, W, C] under the cameras R [N, 3, 3] -> the views [N, h, w, C] on the device.
        ``hfov_deg``: N fields of view, one per frame (``track``), rendered in one launch (``ops.viewport_render_zoom``); with
        ``antialias=True`` every frame has its own ``supersample_for``.  None: the pilot's own, today's call."""
        R = on_device(R, self.device, torch.float32)
        frames = on_device(frames, self.device)
        if hfov_deg is None:
            return ops.viewport_render(frames, R, self.hw, self.hfov_deg, out=out, supersample=self._factor(frames, self.hw))
        fov = self._fovs(hfov_deg, int(frames.shape[0]))
        if self.antialias is True:
            if frames.dim() != 4:
                raise ValueError("frames must be [N, H, W, C], got %s" % (tuple(frames.shape),))
            factors = [supersample_for(frames.shape[1:3], self.hw, v) for v in fov]
        else:
            factors = [self._factor(frames, self.hw)] * len(fov)
        ss = None if all(v == 1 for v in factors) else torch.tensor(factors, dtype=torch.int32).to(self.device)
        return ops.viewport_render_zoom(frames, R, self.hw, ops.viewport_lens(fov, self.hw, device=self.device), out=out,
                                        supersample=ss)

    def outline(self, frames, R, border_px=3, rgb=(0, 255, 0), out=None, hfov_deg=None):
        """frames u8 [N, H, W, 3] -> the panoramas with every view's frame drawn in rgb, on the device.  ``hfov_deg``: as in
        ``render`` (``ops.viewport_outline_zoom``)."""
        frames, R = on_device(frames, self.device), on_device(R, self.device, torch.float32)
        if hfov_deg is None:
            return ops.viewport_outline(frames, R, self.hw, self.hfov_deg, border_px, rgb, out=out, work=self._tab_work(frames))
        if not float(border_px) > 0.0:
            raise ValueError("border_px must be positive, got %r" % (border_px,))
        lens = ops.viewport_lens(self._fovs(hfov_deg, int(frames.shape[0])), self.hw, border_px, device=self.device)
        return ops.viewport_outline_zoom(frames, R, lens, rgb, out=out, work=self._tab_work(frames))

    def agreement(self, R_cam, R, offsets, head=None, hfov_deg=None):
        """The cameras R_cam [F, 3, 3] (``path``) with this pilot's view against the viewers' head cameras R [N, 3, 3], offsets
        [F + 1] (``headtrack.head_cameras``) -> ``headtrack.HeadAgreement``: how much of what the people had in view is in the
        pilot's frame.  ``head``: the ``headtrack.HeadMaps`` that holds the grid and the viewers' window (default: its defaults).
        ``hfov_deg``: F fields of view, one per frame of R_cam (``track``; ``ops.head_agreement_zoom``)."""
        from .headtrack import HeadMaps                                 # headtrack imports look_at from here
        head = head or HeadMaps(device=self.device)
        if hfov_deg is None:
            return head.agreement(R_cam, self.hw, self.hfov_deg, R, offsets)
        return head.agreement(R_cam, self.hw, self._fovs(hfov_deg, len(R_cam)), R, offsets)

    def follow(self, frames, maps, cuts=None):
        """frames u8 [F, H, W, 3], maps f32 [F, hm, wm] (one per frame, e.g. ``SaliencyEngine(.., return_all_steps=True)``'s
        output) -> (views u8 [F, h, w, 3], R f32 [F, 3, 3]) on the device; the frames keep their own resolution.  ``cuts``: as
        in ``path``."""
        frames = on_device(frames, self.device)
        if frames.dim() != 4 or len(maps) != frames.shape[0]:
            raise ValueError("one map per frame: got %d frames and %d maps" % (frames.shape[0], len(maps)))
        R = self.path(maps, cuts)
        return self.render(frames, R), R

    def follow_zoom(self, frames, maps, cuts=None):
        """``follow`` with a field of view per frame: (views [F, h, w, C], R f32 [F, 3, 3] on the device, hfov_deg float64 [F] on
        the host) - ``track``, then ``render`` with its fields of view."""
        frames = on_device(frames, self.device)
        if frames.dim() != 4 or len(maps) != frames.shape[0]:
            raise ValueError("one map per frame: got %d frames and %d maps" % (frames.shape[0], len(maps)))
        R, hfov = self.track(maps, cuts)
        return self.render(frames, R, hfov_deg=hfov), R, hfov

    # ------------------------------------------------------------------------- several cameras at once (K20)
    def paths(self, maps, n, cuts=None, exclude_deg=None, min_share=0.0, arrange='score'):
        """maps f32 [F, hm, wm] -> (R f32 [F, n, 3, 3] on the device, share float64 [n, S] on the host): ``plan_multi``, one
        copy to the host (the directions and the scores together, the one synchronisation of a video) and ``multi_cameras``:
        a camera whose share of camera 0's votes in a shot is below ``min_share`` is dropped there (its R is NaN, its tile
        empty); ``arrange='longitude'`` orders every shot's cameras as the panorama reads, left to right."""
        if not 0.0 <= float(min_share) <= 1.0:
            raise ValueError("min_share must be in [0, 1], got %r" % (min_share,))
        if arrange not in ('score', 'longitude'):
            raise ValueError("arrange must be 'score' or 'longitude', got %r" % (arrange,))
        dirs, score = self.plan_multi(maps, n, cuts, exclude_deg)
        n, F = int(dirs.shape[0]), int(dirs.shape[1])
        both = torch.cat([dirs.reshape(-1).view(torch.int32), score.reshape(-1)]).cpu().numpy()
        R, share = multi_cameras(both[:n * F * 3].view(np.float32).reshape(n, F, 3), both[n * F * 3:].reshape(n, -1), cuts,
                                 self.alpha, self.max_step_deg, min_share, arrange)
        return torch.from_numpy(R.astype(np.float32)).to(self.device), share

    def render_multi(self, frames, R, tiles=None, canvas_hw=None, fill=None, out=None):
        """frames under the cameras R [N, K, 3, 3] -> the canvas [N, hc, wc, C] on the device: camera k's view in tile k
        (``ops.viewport_render_multi``), ``fill`` elsewhere and in the tile of a dropped camera.  The default layout is
        ``split_layout(K, self.hw)``; tiles of other sizes show the same field of view."""
        R = on_device(R, self.device, torch.float32)
        if R.dim() != 4:
            raise ValueError("R must be [N, K, 3, 3], got %s" % (tuple(R.shape),))
        if tiles is None:
            tiles, canvas_hw = split_layout(int(R.shape[1]), self.hw)
        elif canvas_hw is None:
            raise ValueError("tiles need their canvas_hw")
        frames = on_device(frames, self.device)
        tiles = ops.check_tiles(tiles, canvas_hw)[0]
        factors = [self._factor(frames, (h, w)) for _, _, w, h in tiles]
        return ops.viewport_render_multi(frames, R, tiles, self.hfov_deg, canvas_hw, fill=fill, out=out, supersample=factors)

    def follow_multi(self, frames, maps, n, cuts=None, exclude_deg=None, min_share=0.0, arrange='score', tiles=None,
                     canvas_hw=None, fill=None):
        """``follow`` with n cameras: (canvas [F, hc, wc, C], R f32 [F, n, 3, 3]) on the device - ``paths``, then
        ``render_multi``."""
        frames = on_device(frames, self.device)
        if frames.dim() != 4 or len(maps) != frames.shape[0]:
            raise ValueError("one map per frame: got %d frames and %d maps" % (frames.shape[0], len(maps)))
        R = self.paths(maps, n, cuts, exclude_deg, min_share, arrange)[0]
        return self.render_multi(frames, R, tiles, canvas_hw, fill), R

    def outline_multi(self, frames, R, colours=((0, 255, 0), (255, 0, 255), (0, 255, 255), (255, 255, 0), (255, 128, 0),
                                                (0, 128, 255), (255, 0, 0), (255, 255, 255)), border_px=3, out=None):
        """frames u8 [N, H, W, 3] -> the panoramas with the frame of every camera of R [N, K, 3, 3] drawn in its colour, on the
        device: K calls of ``ops.viewport_outline``, all but the first in place.  A dropped camera draws nothing."""
        frames, R = on_device(frames, self.device), on_device(R, self.device, torch.float32)
        if R.dim() != 4 or not 1 <= R.shape[1] <= len(colours):
            raise ValueError("R must be [N, K, 3, 3] with one colour per camera, got %s and %d colours" % (tuple(R.shape), len(colours)))
        work = self._tab_work(frames)
        for k in range(int(R.shape[1])):
            out = ops.viewport_outline(frames if k == 0 else out, R[:, k].contiguous(), self.hw, self.hfov_deg, border_px,
                                       colours[k], out=out, work=work)
        return out

    def agreement_multi(self, R_cam, R, offsets, head=None):
        """The cameras R_cam [F, n, 3, 3] (``paths``) against the viewers' head cameras, as ``agreement`` -> ``MultiAgreement``:
        every viewer is scored against the camera that shows most of what they had in view, so viewers who split between two
        targets no longer count half against the pilot.  ``HeadMaps.agreement`` once per camera, the best of n with torch."""
        from .headtrack import HeadMaps
        head = head or HeadMaps(device=self.device)
        R_cam = on_device(R_cam, self.device, torch.float32)
        if R_cam.dim() != 4 or tuple(R_cam.shape[2:]) != (3, 3) or R_cam.shape[1] < 1:
            raise ValueError("R_cam must be [F, n, 3, 3], got %s" % (tuple(R_cam.shape),))
        F, n = int(R_cam.shape[0]), int(R_cam.shape[1])
        per = [head.agreement(R_cam[:, k].contiguous(), self.hw, self.hfov_deg, R, offsets) for k in range(n)]
        offsets = on_device(offsets, self.device, torch.int32)
        N, dev = int(per[0].iou.shape[0]), per[0].iou.device
        frame = torch.bucketize(torch.arange(N, device=dev, dtype=torch.int32), offsets[1:], right=True).clamp(max=F - 1)
        iou = torch.stack([p.iou for p in per])                                             # [n, N]
        usable = torch.isfinite(R_cam).all(dim=3).all(dim=2).t()[:, frame] & torch.isfinite(iou)
        masked = torch.where(usable, iou, torch.full_like(iou, -1.0))
        top = masked.max(dim=0).values
        first = (masked == top[None, :]).to(torch.int64).argmax(dim=0)                      # the lowest camera on ties
        none = ~usable.any(dim=0)
        best_cam = torch.where(none, torch.full_like(first, -1), first)
        best_iou = torch.where(none, torch.full_like(top, float('nan')), top)
        finite = per[0].finite
        zero = torch.zeros(F, dtype=torch.float64, device=dev)
        total = zero.index_add(0, frame, torch.where(finite, best_iou, torch.zeros_like(best_iou)))
        frame_iou = total / zero.index_add(0, frame, finite.to(torch.float64))
        angles = torch.stack([p.centre_angle_deg for p in per])
        angle = torch.where(none, torch.full_like(top, float('nan')), angles.gather(0, first[None, :])[0])
        return MultiAgreement(best_iou, best_cam, frame_iou, angle, finite, per)
