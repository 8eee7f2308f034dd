"""Shot detection for equirectangular video (K13, csrc/shots.hip): where the hard cuts are.  ``FarnebackFlow``, ``Stabilizer``
and ``ViewportPilot`` assume one continuous take; footage cut from uploads has edits, and the flow of a pair that straddles a cut
means nothing.  The signature of a frame is the colour histogram of the whole sphere with every pixel weighted by its solid angle
(``ops.shot_signatures``): a camera rotation only moves pixels about the sphere, so the signature stays quiet under the motion
``Stabilizer`` removes, and jumps at a cut.  The definition is the package's own (DESIGN.md "K13").

    d_t = sum_{c, b} |sig_t - sig_t+1| / (6 T)   in [0, 1], float64 on the host
    cut between t and t + 1  <=>  d_t >= thr and d_t >= ratio * median(d_s: |s - t| <= radius, s != t)

``find_cuts`` returns the index of the first frame of every new shot, ``segments`` the half-open frame ranges of the shots; a shot
of one frame (a flash) is legal.  ``Stabilizer.rotations / stabilize``, ``smooth_path``, ``cameras`` and ``ViewportPilot.path /
follow`` take the cuts as ``cuts=``; training flows are written shot by shot (``Stabilizer.from_frames`` on every segment of two
frames or more).  Fades, dissolves and cuts between scenes of the same tone are out of scope.
"""
import numpy as np
import torch

from .. import ops
from ._device import host_tensor


def check_cuts(cuts, n):
    """``cuts`` as a list of ints: strictly increasing indices in 1 .. n - 1 (the first frame of every shot but the first) of a
    sequence of n frames, else ValueError.  None -> []."""
    if cuts is None:
        return []
    out = []
    for c in cuts:
        if isinstance(c, (bool, np.bool_)) or not isinstance(c, (int, np.integer)):
            raise ValueError("cuts must be integers, got %r" % (c,))
        c = int(c)
        if not 1 <= c <= int(n) - 1 or (out and c <= out[-1]):
            raise ValueError("cuts must be strictly increasing in 1 .. %d, got %r" % (int(n) - 1, list(cuts)))
        out.append(c)
    return out


def segments(cuts, n):
    """[(lo, hi), ..]: the half-open frame ranges of the shots of an n-frame video, covering 0 .. n."""
    edges = [0] + check_cuts(cuts, n) + [int(n)]
    return list(zip(edges[:-1], edges[1:]))


def find_cuts(d, thr, ratio, radius):
    """d float64 [F - 1], d_t the distance of frames t and t + 1 -> the sorted list of t + 1 (the first frame of each new shot)
    with d_t >= thr and d_t >= ratio * m_t, m_t the median of d_s over s in [t - radius, t + radius] within 0 .. F - 2, s != t
    (0 when there is no such s)."""
    d = np.asarray(d, np.float64).reshape(-1)
    radius = int(radius)
    if radius < 0 or not float(thr) >= 0.0 or not float(ratio) >= 0.0:
        raise ValueError("thr and ratio must not be negative and radius at least 0, got %r, %r, %r" % (thr, ratio, radius))
    cuts = []
    for t in range(d.shape[0]):
        near = np.concatenate([d[max(0, t - radius):t], d[t + 1:t + 1 + radius]])
        m = float(np.median(near)) if near.size else 0.0
        if d[t] >= float(thr) and d[t] >= float(ratio) * m:
            cuts.append(t + 1)
    return cuts


class ShotDetector:
    """``ShotDetector()``: the cuts of u8 [F, H, W, 3] frames at their own resolution.  Holds the weight table and the workspace
    of every (H, W) it has seen.

    The defaults (thr 0.25, ratio 3, radius 8) come from the restatement on the synthetic families of tests/shots_restate.py
    (rotating scenes: d <= 0.07; cuts between scenes of different tone: d >= 0.45); no real footage was available to tune them."""

    def __init__(self, thr=0.25, ratio=3.0, radius=8, device='cuda'):
        if not 0.0 <= float(thr) <= 1.0 or not float(ratio) >= 0.0 or int(radius) < 0:
            raise ValueError("thr must be in [0, 1], ratio not negative and radius at least 0, got %r, %r, %r" % (thr, ratio, radius))
        self.thr, self.ratio, self.radius = float(thr), float(ratio), int(radius)
        self.device = torch.device(device)
        self._geom = {}                          # (H, W) -> [weights (device), T, workspace]

    def _frames(self, frames):
        frames = host_tensor(frames)
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or frames.shape[0] < 1:
            raise ValueError("frames must be uint8 [F, H, W, 3] with F >= 1, got %s %s" % (frames.dtype, tuple(frames.shape)))
        return frames.to(self.device).contiguous()

    def _signatures(self, frames):
        F, H, W = (int(s) for s in frames.shape[:3])
        g = self._geom.get((H, W))
        if g is None:
            a, total = ops.shot_weights_host(H)
            g = self._geom[(H, W)] = [torch.from_numpy(a).to(self.device), W * total, None]
        g[2] = ops._shot_work(F, H, W, frames.device, g[2])
        return ops.shot_signatures(frames, work=g[2], weights=g[0]), g[1]

    def signatures(self, frames):
        """frames u8 [F, H, W, 3] -> sig int64 [F, 3, 64] on the device."""
        return self._signatures(self._frames(frames))[0]

    def distances(self, frames):
        """frames u8 [F, H, W, 3] -> d float64 numpy [F - 1]: the F - 1 sums of absolute differences are copied to the host (the
        one synchronisation) and divided by 6 T there."""
        sig, T = self._signatures(self._frames(frames))
        sad = ops.shot_distances(sig)[0].cpu().numpy()
        return sad.astype(np.float64) / (6.0 * float(T))

    def cuts(self, frames):
        """frames u8 [F, H, W, 3] -> the first frame of every new shot (``find_cuts`` of ``distances``)."""
        return find_cuts(self.distances(frames), self.thr, self.ratio, self.radius)
