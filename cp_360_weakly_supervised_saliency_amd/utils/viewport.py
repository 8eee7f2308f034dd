"""The viewport pilot (K12, csrc/viewport.hip): what a 360-degree saliency map is used for - choosing where to look and rendering
that normal-field-of-view window.  The reference's ``utils/fov_visual.py`` (``box_proh``, ``fov_module``, ``draw_cube_fov_box``)
has this purpose and does not compile; the definition is the package's own (DESIGN.md "K12").

Per frame the saliency map is smoothed on the sphere and its peak refined by one mean-shift step (``ops.sphere_peak``); the peaks
become a smooth camera path on the host (``smooth_path``: a zero-phase exponential filter along great circles; ``look_at``: the
camera with a level horizon), and the views are rendered at the frames' own resolution (``ops.viewport_render``);
``ops.viewport_outline`` draws the view's frame on the panorama.  ``planner='viterbi'`` replaces the per-frame peaks by the path
that collects the most saliency under a turn limit and a turn cost (K16: ``ops.sphere_path``, then ``ops.sphere_refine``): it
chooses which of several targets to follow, where the peaks hop between them.  A camera is a rotation R, camera-to-world, with the columns
(forward, up, right): R = I looks at the panorama's centre.  Roll, translation and anti-aliased views are out of scope.
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


class ViewportPilot:
    """``ViewportPilot((h, w), hfov_deg)``: views of h x w pixels that follow the saliency maps' peak.  Holds the workspaces.

    ``planner``: 'peak', every frame's own peak, or 'viterbi', the best path of K16 under ``turn_cost`` (votes per degree turned;
    a frame's peak votes 4096) and ``plan_step_deg`` (the most the path may turn between two frames).  16 per degree and 15
    degrees are conventions, chosen on the synthetic videos of tests/campath_restate.py and not tuned on data."""

    def __init__(self, hw=(720, 1280), hfov_deg=90.0, sigma_deg=15.0, alpha=0.85, max_step_deg=None, device='cuda', planner='peak',
                 turn_cost=16.0, plan_step_deg=15.0):
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
        self._path_work = ops._work(ops.lib().cp360_path_work_bytes, "sphere_path", F, hm, int(maps.shape[2]), maps.device,
                                    self._path_work, " (F <= 65535, hm wm <= 16384)")
        idx = ops.sphere_path(sm, 4096.0 / val, self.turn_cost, self.plan_step_deg, starts, work=self._path_work)[0]
        return ops.sphere_refine(maps, idx, self.sigma_deg, work=work)

    def path(self, maps, cuts=None):
        """maps f32 [F, hm, wm] -> the cameras R f32 [F, 3, 3] on the device: the peaks (the planned path with the planner
        'viterbi'), copied to the host (3 F floats, the one synchronisation of a video), ``smooth_path`` and ``look_at`` with every
        frame's right chained, copied back.  With ``cuts`` (``utils.shots``) the path of every shot is its own: the concatenation
        of the shots' paths."""
        dirs = (self.plan(maps, cuts) if self.planner == 'viterbi' else self.peaks(maps)).cpu().numpy()
        R = cameras(smooth_path(dirs, self.alpha, self.max_step_deg, cuts), cuts)
        return torch.from_numpy(R.astype(np.float32)).to(self.device)

    def render(self, frames, R, out=None):
        """frames u8 [N, H, W, 3] or f32 [N, H, W, C] under the cameras R [N, 3, 3] -> the views [N, h, w, C] on the device."""
        R = on_device(R, self.device, torch.float32)
        return ops.viewport_render(on_device(frames, self.device), R, self.hw, self.hfov_deg, out=out)

    def outline(self, frames, R, border_px=3, rgb=(0, 255, 0), out=None):
        """frames u8 [N, H, W, 3] -> the panoramas with every view's frame drawn in rgb, on the device."""
        frames, R = on_device(frames, self.device), on_device(R, self.device, torch.float32)
        return ops.viewport_outline(frames, R, self.hw, self.hfov_deg, border_px, rgb, out=out, work=self._tab_work(frames))

    def agreement(self, R_cam, R, offsets, head=None):
        """The cameras R_cam [F, 3, 3] (``path``) with this pilot's view against the viewers' head cameras R [N, 3, 3], offsets
        [F + 1] (``headtrack.head_cameras``) -> ``headtrack.HeadAgreement``: how much of what the people had in view is in the
        pilot's frame.  ``head``: the ``headtrack.HeadMaps`` that holds the grid and the viewers' window (default: its defaults)."""
        from .headtrack import HeadMaps                                 # headtrack imports look_at from here
        head = head or HeadMaps(device=self.device)
        return head.agreement(R_cam, self.hw, self.hfov_deg, R, offsets)

    def follow(self, frames, maps, cuts=None):
        """frames u8 [F, H, W, 3], maps f32 [F, hm, wm] (one per frame, e.g. ``SaliencyEngine(.., return_all_steps=True)``'s
        output) -> (views u8 [F, h, w, 3], R f32 [F, 3, 3]) on the device; the frames keep their own resolution.  ``cuts``: as
        in ``path``."""
        frames = on_device(frames, self.device)
        if frames.dim() != 4 or len(maps) != frames.shape[0]:
            raise ValueError("one map per frame: got %d frames and %d maps" % (frames.shape[0], len(maps)))
        R = self.path(maps, cuts)
        return self.render(frames, R), R
