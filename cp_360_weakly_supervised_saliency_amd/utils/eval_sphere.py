"""Saliency metrics on the sphere, a whole video per call (K14, csrc/sphere_eval.hip): AUC-Judd, NSS, CC, SIM and KL of F
predicted maps against F ground-truth maps, every pixel of the equirectangular evaluation grid weighted by the solid angle of its
row.  ``utils/eval_saliency.py`` (K8) keeps the reference's flat, one-frame functions; the definitions here are the package's own
(DESIGN.md "K14") and tests/sphere_eval_restate.py restates them.

    ev = SphereEval()                                   # 120 x 240, solid-angle weights
    r = ev.evaluate(sal, gt)                            # [F, ., .] numpy or device maps of any size -> SphereScores on the device
    ev.means(r)                                         # {'auc_judd': .., 'nss': .., 'cc': .., 'sim': .., 'kl': ..}, one synchronisation

Maps are resampled to the grid bilinearly on the sphere's pixel centres, without anti-aliasing (as the reference's resize;
``resample='conservative'`` selects K25's conservative remap for ground truth finer than the grid);
fixations are an explicit mask on the grid or the reference's rule ``G > mean + 2 std`` with the same weights.  No jitter, no
random draw: a frame's numbers are bit-identical between runs, batch sizes and places in the batch.  No CPU fallback.
"""
import os
import re

import numpy as np
import torch

from .. import ops
from . import npy_io
from ._device import host_tensor

METRICS = ('auc_judd', 'nss', 'cc', 'sim', 'kl')       # the columns of ops.sphere_eval's scores


class SphereScores:
    """The scores of F frames: ``auc_judd, nss, cc, sim, kl`` float64 [F] and ``n_fix`` int32 [F], all on the device (views of
    ``scores`` float64 [F, 5]); ``frames``: the frame numbers when the maps came from files, else None."""

    def __init__(self, scores, n_fix, frames=None):
        self.scores, self.n_fix, self.frames = scores, n_fix, frames
        for k, name in enumerate(METRICS):
            setattr(self, name, scores[:, k])

    def __len__(self):
        return int(self.scores.shape[0])


class SphereEval:
    """``SphereEval(grid_hw=(120, 240), weights='solid_angle')``: holds the weight table of the grid and the workspace, which
    grows to the longest video seen.  ``weights='uniform'`` scores a flat grid, as the reference does.  ``resample='conservative'``
    brings maps finer than the grid down by the conservative remap (K25, ``ops.sphere_resample``: every source pixel is read, the
    mass on the sphere is kept) instead of the four bilinear taps, which stay the default."""

    def __init__(self, grid_hw=(120, 240), weights='solid_angle', device='cuda', resample='bilinear'):
        h, w = (int(v) for v in grid_hw)
        self.resampler = ops.check_resampler(resample)
        if h < 1 or w < 1 or h * w > 1 << 21:
            raise ValueError("the grid must be between 1 x 1 and 2^21 pixels, got %d x %d" % (h, w))
        if weights not in ('solid_angle', 'uniform'):
            raise ValueError("weights must be 'solid_angle' or 'uniform', got %r" % (weights,))
        self.grid_hw, self.mode, self.device = (h, w), weights, torch.device(device)
        self._weights = None
        self._work = None

    @property
    def weights(self):
        if self._weights is None:
            self._weights = ops.sphere_eval_weights(self.grid_hw[0], self.mode, self.device)
        return self._weights

    def _maps(self, name, maps):
        maps = host_tensor(maps, np.float32)
        if maps.dim() != 3 or maps.shape[0] < 1 or not maps.dtype.is_floating_point:
            raise ValueError("%s must be floating-point [F, h, w] with F >= 1, got %s %s" % (name, maps.dtype, tuple(maps.shape)))
        return maps.detach().to(self.device, torch.float32).contiguous()

    def resample(self, maps):
        """maps [F, hs, ws] (numpy or tensor) -> float32 [F, h, w] on the device, on the evaluation grid."""
        return ops.resample_maps(self._maps('maps', maps), self.grid_hw, self.resampler)

    def evaluate(self, sal, gt, fixations=None):
        """sal [F, ., .], gt [F, ., .] (numpy or tensors, any sizes) and, optionally, fixations [F, h, w] on the grid (non-zero =
        fixated; default: ``G > mean + 2 std``) -> ``SphereScores``.  Nothing is copied back and nothing waits."""
        S, G = self.resample(sal), self.resample(gt)
        if S.shape[0] != G.shape[0]:
            raise ValueError("sal and gt must have as many frames, got %d and %d" % (S.shape[0], G.shape[0]))
        if fixations is not None:
            fixations = host_tensor(fixations)
            if fixations.dtype not in (torch.uint8, torch.bool):
                fixations = fixations != 0
            fixations = fixations.to(self.device).contiguous()
        self._work = ops.sphere_eval_work(S.shape[0], self.grid_hw[0], self.grid_hw[1], S.device, self._work)
        scores, n_fix = ops.sphere_eval(S, G, self.weights, fixations, work=self._work)
        return SphereScores(scores, n_fix)

    def means(self, result):
        """The plain mean of every metric over the frames (NaN frames included, as ``np.mean`` in the reference's test loop) ->
        {name: float}; one copy to the host, the only synchronisation."""
        m = result.scores.mean(dim=0).cpu().numpy()
        return {name: float(m[k]) for k, name in enumerate(METRICS)}


def dataset_means(per_video_means, frame_counts):
    """The reference's dataset figure: the mean of the per-video means weighted by the videos' frame counts.  per_video_means:
    a list of ``SphereEval.means`` dicts -> {name: float}."""
    counts = np.asarray(frame_counts, np.float64).reshape(-1)
    if len(per_video_means) != counts.shape[0] or counts.shape[0] < 1 or not np.all(counts > 0):
        raise ValueError("one positive frame count per video, got %d means and counts %r" % (len(per_video_means), frame_counts))
    total = counts.sum()
    return {name: float(np.sum([m[name] * c / total for m, c in zip(per_video_means, counts)])) for name in METRICS}


def evaluate_video_dir(pred_dir, gt_dir, vid_name, evaluator=None):
    """Scores the saliency maps a run left on disk: every ``<pred_dir>/<vid_name>/{:05}.npy`` (``npy_io.saliency_path``) against
    ``<gt_dir>/<vid_name>.mp4/{:05}.npy`` of the same number, in ascending order, in one call -> ``SphereScores`` with
    ``frames`` = the numbers.  A prediction without ground truth is an error.  The maps are resampled as the evaluator does:
    ``evaluator=SphereEval(resample='conservative')`` for ground truth much finer than the grid."""
    ev = evaluator or SphereEval()
    vdir = os.path.join(pred_dir, vid_name)
    numbers = sorted(int(n[:-4]) for n in os.listdir(vdir) if re.fullmatch(r'\d{5}\.npy', n))
    if not numbers:
        raise FileNotFoundError("no saliency maps ({:05}.npy) in %s" % vdir)
    sal = np.stack([np.load(npy_io.saliency_path(pred_dir, vid_name, n)) for n in numbers])
    gt = np.stack([np.load(npy_io.saliency_path(gt_dir, vid_name + '.mp4', n)) for n in numbers])
    r = ev.evaluate(sal, gt)
    r.frames = numbers
    return r
