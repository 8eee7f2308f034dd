"""Ground truth from head tracking (K17, csrc/headtrack.hip).  Most 360-degree datasets log the head's orientation only: what a
viewer saw is then the window of the headset, not a point.  A viewer is a camera in the viewport pilot's convention (a rotation R,
camera-to-world, columns forward / up / right), and two things are built from the viewers' windows: the ground-truth map, the
share of the viewers who had a pixel in view, and a score for a virtual camera, how much of what the people looked at is in its
frame.  The definitions are the package's own (DESIGN.md "K17") and tests/headtrack_restate.py restates them.

    R, offsets, viewer = head_cameras(tracks, fps=30.0, n_frames=F)          # host, float64 -> float32
    hm = HeadMaps()                                                           # 120 x 240, a square window of 100 degrees
    gt = hm.coverage(R, offsets)                                              # f32 [F, 120, 240]: SphereEval, save_gt
    res = hm.agreement(pilot.path(maps), pilot.hw, pilot.hfov_deg, R, offsets)
    hm.means(res)                                                             # {'iou': .., 'centre_angle_deg': .., ..}

The window of 100 degrees, square, is a convention for headsets: it has not been tuned on a dataset.  No CPU fallback for the
maps and the score; the interpolation of the tracks is host numpy, ``fixations.scanpaths_to_points``' own.
"""
import numpy as np
import torch

from .. import ops
from ._device import on_device
from .fixations import _frame_times, _track_directions
from .viewport import look_at

_TWO_PI = 2.0 * np.pi


def head_cameras(tracks, fps, n_frames, max_gap=0.5):
    """tracks: one ``(t, lon, lat)`` or ``(t, lon, lat, roll)`` per viewer, t in seconds ascending, angles in radians -> (R
    float32 [N, 3, 3], offsets int32 [n_frames + 1], viewer int32 [N]), frame by frame, viewers in their order; viewer[k] is the
    track that camera k comes from.  The direction at (f + 0.5) / fps and the frames a viewer is dropped from are exactly
    ``scanpaths_to_points``'; the roll is interpolated linearly along the shorter arc, and a frame whose roll is not finite is
    dropped too.  The camera is ``viewport.look_at`` of the direction, every viewer's previous right handed on for the poles,
    then rolled about its forward axis: up' = cos r up + sin r right, right' = -sin r up + cos r right."""
    tf, max_gap = _frame_times(fps, n_frames, max_gap)
    F = tf.size
    cams = np.full((len(tracks), F, 3, 3), np.nan)
    for v, track in enumerate(tracks):
        if len(track) not in (3, 4):
            raise ValueError("viewer %d: a track is (t, lon, lat) or (t, lon, lat, roll), got %d arrays" % (v, len(track)))
        found = _track_directions(v, track[0], track[1], track[2], tf, max_gap)
        if found is None:
            continue
        p, ok, i0, i1, s = found
        roll = np.zeros(F)
        if len(track) == 4:
            r = np.asarray(track[3], np.float64).reshape(-1)
            if r.size != np.asarray(track[0]).size:
                raise ValueError("viewer %d: roll must be as long as t, got %d" % (v, r.size))
            with np.errstate(invalid='ignore'):
                d = np.mod(r[i1] - r[i0] + np.pi, _TWO_PI) - np.pi       # the shorter way round, in [-pi, pi)
                roll = r[i0] + s * d
            ok = ok & np.isfinite(roll)
        kept = np.flatnonzero(ok)
        if kept.size == 0:
            continue
        f = p[kept]
        f = f / np.linalg.norm(f, axis=-1, keepdims=True)
        right = np.stack([-f[:, 2], np.zeros(kept.size), f[:, 0]], axis=-1)                # f x (0, 1, 0)
        norm = np.linalg.norm(right, axis=-1)
        pole = norm < 1e-6
        right[~pole] /= norm[~pole, None]
        for j in np.flatnonzero(pole):                                 # in ascending order: the right before it is final
            right[j] = look_at(f[j], right[j - 1] if j > 0 else None)[:, 2]
        up = np.cross(right, f)
        c, sn = np.cos(roll[kept])[:, None], np.sin(roll[kept])[:, None]
        cams[v, kept] = np.stack([f, c * up + sn * right, c * right - sn * up], axis=-1)
    keep = np.isfinite(cams[:, :, 0, 0]).T                              # [F, V]: frame by frame, viewers in order
    offsets = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int32)
    R = np.ascontiguousarray(cams.transpose(1, 0, 2, 3)[keep].astype(np.float32).reshape(-1, 3, 3))
    viewer = np.broadcast_to(np.arange(len(tracks), dtype=np.int32)[None, :], keep.shape)[keep]
    return R, offsets, np.ascontiguousarray(viewer, dtype=np.int32)


class HeadAgreement:
    """What ``HeadMaps.agreement`` returns, on the device: ``inter`` and ``union`` int64 [N], the weighted pixels inside both
    windows and inside either; ``iou`` float64 [N], their exact quotient (NaN where the union is 0); ``frame_iou`` float64 [F],
    the mean over the frame's finite viewers (NaN without any); ``centre_angle_deg`` float64 [N], the angle between the two
    forward axes; ``finite`` bool [N], the viewers whose camera is finite."""

    def __init__(self, inter, union, iou, frame_iou, centre_angle_deg, finite):
        self.inter, self.union, self.iou, self.frame_iou = inter, union, iou, frame_iou
        self.centre_angle_deg, self.finite = centre_angle_deg, finite


class HeadMaps:
    """``HeadMaps(grid_hw=(120, 240), view_hw=(1, 1), hfov_deg=100.0)``: the viewers' windows on one grid - footprint counts,
    the coverage map and the agreement of a camera with the viewers.  Every viewer has the view (view_hw, hfov_deg): only the
    ratio of view_hw counts.  100 degrees and square are a convention for headsets, not tuned on data.  Holds the workspace."""

    def __init__(self, grid_hw=(120, 240), view_hw=(1, 1), hfov_deg=100.0, device='cuda'):
        h, w = (int(v) for v in grid_hw)
        if h < 1 or w < 1 or h * w > 1 << 21:
            raise ValueError("the grid must be between 1 x 1 and 2^21 pixels, got %d x %d" % (h, w))
        ops._head_view(view_hw, hfov_deg)
        self.grid_hw, self.view_hw, self.hfov_deg = (h, w), (float(view_hw[0]), float(view_hw[1])), float(hfov_deg)
        self.device = torch.device(device)
        self._work = None

    def _cameras(self, R, offsets):
        R = on_device(R, self.device, torch.float32).reshape(-1, 3, 3)
        return R, on_device(offsets, self.device, torch.int32)

    def _workspace(self, device):
        self._work = ops.head_work(self.grid_hw[0], self.grid_hw[1], device, self._work)
        return self._work

    def footprints(self, R, offsets):
        """-> (counts int32 [F, h, w], n_views int32 [F]) on the device."""
        R, offsets = self._cameras(R, offsets)
        return ops.head_footprints(R, offsets, self.grid_hw, self.view_hw, self.hfov_deg, work=self._workspace(R.device))

    def coverage(self, R, offsets):
        """-> float32 [F, h, w] = counts / max(n_views, 1), the share of the frame's viewers who had the pixel in view: the
        ground-truth map, as ``SphereEval.evaluate`` and ``fixations.save_gt`` take it.  A frame without viewers is zero."""
        counts, n_views = self.footprints(R, offsets)
        return counts.to(torch.float32) / n_views.clamp(min=1).to(torch.float32)[:, None, None]

    def agreement(self, R_cam, cam_hw, cam_hfov_deg, R, offsets, weights='solid_angle'):
        """The camera R_cam [F, 3, 3] (``ViewportPilot.path``) with views of cam_hw and cam_hfov_deg against every viewer of its
        frame -> ``HeadAgreement``.  weights: 'solid_angle' (areas on the sphere) or 'uniform' (pixels of the grid times 1024).
        cam_hfov_deg may be F values, a field of view per frame of R_cam (K22c, ``ops.head_agreement_zoom``)."""
        R, offsets = self._cameras(R, offsets)
        R_cam = on_device(R_cam, R.device, torch.float32)
        a = ops.sphere_eval_weights(self.grid_hw[0], weights, R.device)
        if np.ndim(cam_hfov_deg) == 0:
            inter, union = ops.head_agreement(R_cam, (cam_hw, cam_hfov_deg), R, offsets, self.grid_hw, (self.view_hw, self.hfov_deg),
                                              a, work=self._workspace(R.device))
        else:                                                           # K22c: a field of view per frame of R_cam
            lens = ops.viewport_lens(cam_hfov_deg, cam_hw, device=R.device, n=len(R_cam))
            inter, union = ops.head_agreement_zoom(R_cam, lens, R, offsets, self.grid_hw, (self.view_hw, self.hfov_deg), a,
                                                   work=self._workspace(R.device))
        N, F = int(R.shape[0]), int(offsets.shape[0]) - 1
        iou = inter.to(torch.float64) / union.to(torch.float64)                             # 0 / 0 = NaN
        frame = torch.bucketize(torch.arange(N, device=R.device, dtype=torch.int32), offsets[1:], right=True).clamp(max=F - 1)
        finite = torch.isfinite(R).all(dim=2).all(dim=1)
        zero = torch.zeros(F, dtype=torch.float64, device=R.device)
        total = zero.index_add(0, frame, torch.where(finite, iou, torch.zeros_like(iou)))
        frame_iou = total / zero.index_add(0, frame, finite.to(torch.float64))              # no finite viewer: 0 / 0 = NaN
        fc, fv = R_cam.to(torch.float64)[frame][:, :, 0], R.to(torch.float64)[:, :, 0]
        angle = torch.rad2deg(torch.atan2(torch.linalg.cross(fc, fv, dim=1).norm(dim=1), (fc * fv).sum(dim=1)))
        return HeadAgreement(inter, union, iou, frame_iou, angle, finite)

    @staticmethod
    def means(result):
        """The video's figures, copied to the host: {'iou': the mean of ``frame_iou`` over the frames that have one,
        'centre_angle_deg': the mean over the finite viewers, 'frames': the frames with a viewer, 'pairs': the finite viewers}."""
        has = ~torch.isnan(result.frame_iou)
        fin = result.finite & ~torch.isnan(result.centre_angle_deg)
        n_f, n_p = int(has.sum()), int(fin.sum())
        return {'iou': float(result.frame_iou[has].mean()) if n_f else float('nan'),
                'centre_angle_deg': float(result.centre_angle_deg[fin].mean()) if n_p else float('nan'),
                'frames': n_f, 'pairs': n_p}
