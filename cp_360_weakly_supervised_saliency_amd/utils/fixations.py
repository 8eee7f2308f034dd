"""Fixation ground truth from scan-paths, and shuffled AUC on the sphere (K15, csrc/fixations.hip).  Head- or eye-tracking logs
(per viewer: time, longitude, latitude) become per-frame fixation points, counts, masks and density maps on the equirectangular
grid, blurred on the sphere and not on the flat image, and saved where ``eval_sphere.evaluate_video_dir`` reads ground truth.  The
definitions are the package's own (DESIGN.md "K15") and tests/fixations_restate.py restates them.

    lonlat, offsets = scanpaths_to_points(tracks, fps=30.0, n_frames=F)      # host, float64
    fm = FixationMaps()                                                       # 120 x 240, sigma 5 degrees
    gt = fm.density(lonlat, offsets)                                          # f32 [F, 120, 240] on the device
    save_gt(gt_dir, vid_name, gt)                                             # <gt_dir>/<vid_name>.mp4/{:05}.npy
    counts, _ = fm.counts(lonlat, offsets)
    auc, c_tot, a_neg = fm.shuffled_auc(sal, counts)                          # negatives: the other frames' fixations
    top = fm.ceiling(lonlat, offsets)                                         # K19: the other viewers predict the one left out
    mine = fm.score_points(sal, lonlat, offsets)                              # the same scores of a model's maps: .video_auc, ..
    rows = fm.baselines(lonlat, offsets, sal)                                 # 'ceiling', 'prior', 'model', 'normalised'

The ceiling and the point scores (K19) take the points of one frame as different viewers', which is what ``scanpaths_to_points``
gives: at most one point per viewer and frame.  Longitude is theta and latitude phi of the package's sphere geometry (north up, radians).  ``sigma_deg = 5`` is a convention: it
has not been tuned on a dataset.  No CPU fallback for the maps and the score; the scan-path interpolation is host numpy.
"""
import collections
import os

import numpy as np
import torch

from .. import ops
from . import npy_io
from ._device import host_tensor, on_device


POINT_CHUNK = 256                                                      # K19: frames per call, 59 MB of workspace on 120 x 240
PointScores = collections.namedtuple('PointScores', 'auc nss frame_auc frame_nss video_auc video_nss')


def _unit(lon, lat):
    cl = np.cos(lat)
    return np.stack([cl * np.cos(lon), np.sin(lat), cl * np.sin(lon)], axis=-1)


def _frame_times(fps, n_frames, max_gap):
    """The checks of the scan-path functions -> (the frames' times (f + 0.5) / fps float64 [n_frames], max_gap)."""
    fps, n_frames, max_gap = float(fps), int(n_frames), float(max_gap)
    if not fps > 0.0 or n_frames < 1 or not max_gap >= 0.0:
        raise ValueError("fps > 0, n_frames >= 1 and max_gap >= 0 are needed, got %r, %r, %r" % (fps, n_frames, max_gap))
    return (np.arange(n_frames, dtype=np.float64) + 0.5) / fps, max_gap


def _track_directions(v, t, lon, lat, tf, max_gap):
    """Viewer v's direction at the times tf: (p float64 [F, 3], ok bool [F], i0, i1 int [F], s float64 [F]) - the unit direction
    by spherical linear interpolation between the samples i0 and i1 at the fraction s, and whether the viewer gives one to the
    frame; None for an empty track.  ``scanpaths_to_points`` and ``headtrack.head_cameras`` both take their directions from here."""
    t, lon, lat = (np.asarray(a, np.float64).reshape(-1) for a in (t, lon, lat))
    if not (t.shape == lon.shape == lat.shape):
        raise ValueError("viewer %d: t, lon and lat must be as long, got %d, %d, %d" % (v, t.size, lon.size, lat.size))
    if t.size == 0:
        return None
    if np.any(np.diff(t) < 0.0) or not np.all(np.isfinite(t)):
        raise ValueError("viewer %d: t must be finite and ascending" % v)
    i1 = np.searchsorted(t, tf, side='left')                           # the first sample at or after the frame's time
    inside = (tf >= t[0]) & (tf <= t[-1])
    i1 = np.clip(i1, 0, t.size - 1)
    i0 = np.where(t[i1] == tf, i1, np.maximum(i1 - 1, 0))              # on a sample: that sample alone
    dt = t[i1] - t[i0]
    ok = inside & (dt <= max_gap)
    a, b = _unit(lon[i0], lat[i0]), _unit(lon[i1], lat[i1])
    with np.errstate(all='ignore'):
        s = np.where(dt > 0.0, (tf - t[i0]) / np.where(dt > 0.0, dt, 1.0), 0.0)
        omega = np.arctan2(np.linalg.norm(np.cross(a, b), axis=-1), np.sum(a * b, axis=-1))
        so = np.sin(omega)
        small = so < 1e-12                                             # the same direction (or opposite ones: no great circle)
        wa = np.where(small, 1.0 - s, np.sin((1.0 - s) * omega) / np.where(small, 1.0, so))
        wb = np.where(small, s, np.sin(s * omega) / np.where(small, 1.0, so))
        p = wa[:, None] * a + wb[:, None] * b
        p = p / np.linalg.norm(p, axis=-1, keepdims=True)
    ok &= np.all(np.isfinite(p), axis=-1)
    return p, ok, i0, i1, s


def scanpaths_to_points(tracks, fps, n_frames, max_gap=0.5):
    """tracks: one ``(t, lon, lat)`` per viewer, t in seconds ascending, angles in radians -> (lonlat float64 [N, 2], offsets
    int32 [n_frames + 1]), frame by frame, viewers in their order.  Frame f takes each viewer's direction at (f + 0.5) / fps by
    spherical linear interpolation between the two bracketing samples; a viewer gives no point to a frame outside the track's
    span, between samples more than max_gap seconds apart, or between samples that are not finite."""
    tf, max_gap = _frame_times(fps, n_frames, max_gap)
    n_frames = tf.size
    lon_out = np.full((len(tracks), n_frames), np.nan)
    lat_out = np.full((len(tracks), n_frames), np.nan)
    for v, (t, lon, lat) in enumerate(tracks):
        found = _track_directions(v, t, lon, lat, tf, max_gap)
        if found is None:
            continue
        p, ok = found[:2]
        lon_out[v, ok] = np.arctan2(p[ok, 2], p[ok, 0])
        lat_out[v, ok] = np.arcsin(np.clip(p[ok, 1], -1.0, 1.0))
    keep = np.isfinite(lon_out).T                                      # [F, V]: frame by frame, viewers in order
    offsets = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int32)
    lonlat = np.stack([lon_out.T[keep], lat_out.T[keep]], axis=-1).astype(np.float64).reshape(-1, 2)
    return np.ascontiguousarray(lonlat), offsets


class FixationMaps:
    """``FixationMaps(grid_hw=(120, 240), sigma_deg=5.0)``: fixation counts, masks, density maps and shuffled AUC on one grid; holds
    the workspace, which grows to the longest video seen.  ``resample='conservative'`` brings saliency maps finer than the grid down
    by the conservative remap (K25, ``ops.sphere_resample``) instead of the bilinear taps, as ``SphereEval`` does."""

    def __init__(self, grid_hw=(120, 240), sigma_deg=5.0, device='cuda', resample='bilinear'):
        h, w = (int(v) for v in grid_hw)
        self.resampler = ops.check_resampler(resample)
        if h < 1 or w < 1 or h * w > 1 << 21:
            raise ValueError("the grid must be between 1 x 1 and 2^21 pixels, got %d x %d" % (h, w))
        sigma_deg = float(sigma_deg)
        if not (sigma_deg > 0.0 and np.isfinite(sigma_deg)):
            raise ValueError("sigma_deg must be finite and positive, got %r" % (sigma_deg,))
        self.grid_hw, self.sigma_deg, self.device = (h, w), sigma_deg, torch.device(device)
        self._work = None

    def _points(self, lonlat, offsets):
        if not torch.is_tensor(lonlat):
            lonlat = torch.from_numpy(np.ascontiguousarray(lonlat, dtype=np.float64).reshape(-1, 2))
        return on_device(lonlat, self.device, torch.float64), on_device(offsets, self.device, torch.int32)

    def _workspace(self, F, device):
        """The workspace for F frames on `device` (a tensor's, with its index); kept while it is large enough."""
        self._work = ops.fixation_work(F, self.grid_hw[0], self.grid_hw[1], device, self._work)
        return self._work

    def counts(self, lonlat, offsets):
        """-> (counts int32 [F, h, w], n_points int32 [F]) on the device."""
        lonlat, offsets = self._points(lonlat, offsets)
        return ops.fixation_counts(lonlat, offsets, self.grid_hw)

    def mask(self, lonlat, offsets):
        """-> uint8 [F, h, w], 1 where a pixel holds a fixation: ``SphereEval.evaluate(sal, gt, fixations=mask)``."""
        return (self.counts(lonlat, offsets)[0] > 0).to(torch.uint8)

    def density(self, lonlat, offsets, normalize='max'):
        """-> float32 [F, h, w]: every point blurred on the sphere with sigma_deg.  normalize: 'max' (every frame's maximum is 1),
        'mass' (every frame's solid-angle-weighted sum, with K13's row weights / 1024, is 1) or None; a frame without points
        stays zero."""
        if normalize not in ('max', 'mass', None):
            raise ValueError("normalize must be 'max', 'mass' or None, got %r" % (normalize,))
        lonlat, offsets = self._points(lonlat, offsets)
        G = ops.fixation_density(lonlat, offsets, self.grid_hw, np.deg2rad(self.sigma_deg), work=self._workspace(0, lonlat.device))
        if normalize is None:
            return G
        if normalize == 'max':
            d = G.amax(dim=(1, 2))
        else:
            a = ops.sphere_eval_weights(self.grid_hw[0], 'solid_angle', G.device).to(torch.float64) / 1024.0
            d = (G.to(torch.float64) * a[None, :, None]).sum(dim=(1, 2)).to(torch.float32)
        return G / torch.where(d > 0, d, torch.ones_like(d))[:, None, None]

    def shuffled_auc(self, sal, counts, negatives='other_frames'):
        """sal [F, ., .] (numpy or tensor, any size: resampled to the grid as ``SphereEval`` does), counts int32 [F, h, w] ->
        (auc float64 [F], c_tot int64 [F], a_neg int64 [F]) on the device.  negatives: 'other_frames' (frame f draws its negatives
        from the fixations of every other frame of the video) or an [h, w] count map for every frame."""
        sal = host_tensor(sal, np.float32)
        if sal.dim() != 3 or sal.shape[0] < 1 or not sal.dtype.is_floating_point:
            raise ValueError("sal must be floating-point [F, h, w] with F >= 1, got %s %s" % (sal.dtype, tuple(sal.shape)))
        S = ops.resample_maps(sal.detach().to(self.device, torch.float32).contiguous(), self.grid_hw, self.resampler)
        counts = host_tensor(counts)
        F, (h, w) = int(S.shape[0]), self.grid_hw
        if tuple(counts.shape) != (F, h, w) or counts.dtype.is_floating_point:
            raise ValueError("counts must be integers [%d, %d, %d], got %s %s" % (F, h, w, counts.dtype, tuple(counts.shape)))
        pos = counts.to(self.device, torch.int32).contiguous()
        if isinstance(negatives, str):
            if negatives != 'other_frames':
                raise ValueError("negatives must be 'other_frames' or an [h, w] count map, got %r" % (negatives,))
            neg = (pos.sum(dim=0, keepdim=True, dtype=torch.int64) - pos).clamp(max=1 << 20).to(torch.int32)
        else:
            negatives = host_tensor(negatives)
            if tuple(negatives.shape) != (h, w) or negatives.dtype.is_floating_point:
                raise ValueError("negatives must be integers [%d, %d], got %s %s" % (h, w, negatives.dtype, tuple(negatives.shape)))
            neg = negatives.to(self.device, torch.int32).reshape(1, h, w).contiguous()
        return ops.shuffled_auc(S, pos, neg.contiguous(), work=self._workspace(F, S.device))

    # ------------------------------------------------------------------------- K19: the ceiling and the baselines
    def _score(self, lonlat, offsets, weights, sal):
        """The point scores of a video, POINT_CHUNK frames a call -> PointScores.  sal None: leave-one-out."""
        h, w = self.grid_hw
        off = (offsets.detach().cpu().numpy() if torch.is_tensor(offsets) else np.asarray(offsets)).astype(np.int64).reshape(-1)
        if not torch.is_tensor(lonlat):
            lonlat = torch.from_numpy(np.array(lonlat, dtype=np.float64).reshape(-1, 2))       # a copy: the caller's may be read-only
        N, F = int(lonlat.shape[0]), off.size - 1
        if lonlat.dim() != 2 or lonlat.shape[1] != 2 or F < 1 or np.any(np.diff(off) < 0) or off[0] < 0 or off[-1] > N:
            raise ValueError("lonlat must be [N, 2] and offsets [F + 1] with F >= 1, ascending within 0 .. N")
        if weights not in ('solid_angle', 'uniform'):
            raise ValueError("weights must be 'solid_angle' or 'uniform', got %r" % (weights,))
        if sal is not None:
            sal = host_tensor(sal, np.float32)
            if not sal.dtype.is_floating_point or not (sal.dim() == 2 or (sal.dim() == 3 and sal.shape[0] == F)) or sal.numel() == 0:
                raise ValueError("sal must be floating-point [%d, h, w] or one [h, w] map, got %s %s" % (F, sal.dtype, tuple(sal.shape)))
        lonlat = on_device(lonlat, self.device, torch.float64)
        dev = lonlat.device
        a = ops.sphere_eval_weights(h, weights, dev)
        one = None
        if sal is not None and sal.dim() == 2:
            one = ops.resample_maps(sal.detach()[None].to(dev, torch.float32).contiguous(), self.grid_hw, self.resampler)
        scores = torch.full((N, 2), float('nan'), dtype=torch.float64, device=dev)
        for c0 in range(0, F, POINT_CHUNK):
            c1 = min(F, c0 + POINT_CHUNK)
            k0, k1 = int(off[c0]), int(off[c1])
            if k1 == k0:
                continue
            offs = torch.from_numpy((off[c0:c1 + 1] - k0).astype(np.int32)).to(dev)
            self._work = ops.fixation_point_work(c1 - c0, h, w, dev, self._work)
            if sal is None:
                part = ops.fixation_point_scores(lonlat[k0:k1], offs, self.grid_hw, a, sigma_rad=np.deg2rad(self.sigma_deg), work=self._work)
            else:
                maps = one if one is not None else ops.resample_maps(
                    sal[c0:c1].detach().to(dev, torch.float32).contiguous(), self.grid_hw, self.resampler)
                part = ops.fixation_point_scores(lonlat[k0:k1], offs, self.grid_hw, a, maps=maps, work=self._work)
            scores[k0:k1] = part
        # the means: a frame's points are consecutive, one segment each, added in their order
        lengths = torch.from_numpy(np.diff(off)).to(dev)
        owned = scores[int(off[0]):int(off[-1])]
        out = []
        for c in range(2):
            v = owned[:, c].contiguous()
            ok = ~torch.isnan(v)
            tot = torch.segment_reduce(torch.where(ok, v, torch.zeros_like(v)), 'sum', lengths=lengths, unsafe=True)
            cnt = torch.segment_reduce(ok.to(torch.float64), 'sum', lengths=lengths, unsafe=True)
            out.append((tot / cnt, tot.sum() / cnt.sum()))                 # 0 / 0: NaN for a frame, or a video, without a number
        return PointScores(scores[:, 0], scores[:, 1], out[0][0], out[1][0], out[0][1], out[1][1])

    def ceiling(self, lonlat, offsets, weights='solid_angle'):
        """The human ceiling (inter-observer consistency): every point scored against the density of the other points of its
        frame, blurred with sigma_deg - how well the other viewers predict the one left out.  The points of one frame are taken
        as different viewers', which is what ``scanpaths_to_points`` gives: at most one point per viewer and frame.  -> PointScores
        on the device: auc, nss f64 [N]; frame_auc, frame_nss f64 [F], the mean over the frame's points that have a number (NaN
        for a frame with none: a viewer alone has an AUC of 1/2 and no NSS); video_auc, video_nss, the mean over all points that
        have one.  weights: 'solid_angle' or 'uniform', as ``SphereEval``.  The video goes through in chunks of POINT_CHUNK
        frames, which bounds the workspace; a point's bits do not depend on the chunking."""
        return self._score(lonlat, offsets, weights, None)

    def score_points(self, sal, lonlat, offsets, weights='solid_angle'):
        """The same scores of maps: sal [F, ., .] (numpy or tensor, any size: resampled to the grid as ``SphereEval`` does) or
        one [., .] map for every frame; every point of frame f is scored against sal[f] -> PointScores, in the units of
        ``ceiling``."""
        if sal is None:
            raise ValueError("sal must be [F, h, w] or one [h, w] map")
        return self._score(lonlat, offsets, weights, sal)

    def prior(self, lonlat, offsets, exclude_own=True):
        """The prior baseline, a map that has never seen the frame: float32 [F, h, w], for frame f the mean of the other frames'
        raw densities, (sum_g D_g - D_f) / (F - 1), summed in float64; exclude_own=False: the [h, w] mean of all frames."""
        D = self.density(lonlat, offsets, None)
        F = int(D.shape[0])
        tot = D.sum(dim=0, dtype=torch.float64)
        if not exclude_own:
            return (tot / F).to(torch.float32)
        if F < 2:
            raise ValueError("the prior of the other frames needs F >= 2 (or exclude_own=False)")
        out = torch.empty_like(D)
        for c0 in range(0, F, POINT_CHUNK):
            out[c0:c0 + POINT_CHUNK] = ((tot[None] - D[c0:c0 + POINT_CHUNK]).clamp_(min=0.0) / (F - 1)).to(torch.float32)
        return out

    def baselines(self, lonlat, offsets, sal=None):
        """The reference lines of a report -> {'ceiling': (video_auc, video_nss), 'prior': ..} and, when sal is given, 'model' and
        'normalised' = (model - prior) / (ceiling - prior) per score: 0 at the prior, 1 at the ceiling.  'prior' is
        ``score_points(prior(lonlat, offsets), ..)``, the other frames' densities; 0-dim float64 tensors on the device."""
        rows = {}
        for name, r in (('ceiling', self.ceiling(lonlat, offsets)),
                        ('prior', self.score_points(self.prior(lonlat, offsets), lonlat, offsets))):
            rows[name] = (r.video_auc, r.video_nss)
        if sal is not None:
            r = self.score_points(sal, lonlat, offsets)
            rows['model'] = (r.video_auc, r.video_nss)
            rows['normalised'] = tuple((m - p) / (c - p) for m, p, c in zip(rows['model'], rows['prior'], rows['ceiling']))
        return rows


def save_gt(gt_dir, vid_name, maps, first_frame_no=0):
    """Writes maps [F, h, w] (numpy or tensor) as ``<gt_dir>/<vid_name>.mp4/{:05}.npy``, float32, numbered from first_frame_no:
    where ``eval_sphere.evaluate_video_dir`` and the reference's test loop read ground truth.  -> the paths."""
    if torch.is_tensor(maps):
        maps = maps.detach().cpu().numpy()
    maps = np.asarray(maps, np.float32)
    if maps.ndim != 3 or maps.shape[0] < 1:
        raise ValueError("maps must be [F, h, w] with F >= 1, got %s" % (maps.shape,))
    first_frame_no = int(first_frame_no)
    if first_frame_no < 0 or first_frame_no + maps.shape[0] > 100000:
        raise ValueError("frame numbers must stay within 0 .. 99999, got %d .. %d" % (first_frame_no, first_frame_no + maps.shape[0] - 1))
    paths = []
    for k in range(maps.shape[0]):
        path = npy_io.saliency_path(gt_dir, vid_name + '.mp4', first_frame_no + k)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        np.save(path, maps[k])
        paths.append(path)
    return paths
