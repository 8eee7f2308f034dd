"""Optical flow of /root/reference/utils/optical_flow.py on the device: ``calcOpticalFlow`` with the reference's name and
signature, computed by Farneback's method (K10, csrc/optflow.hip) - the ``cv2.calcOpticalFlowFarneback(prev, cur, None, 0.5,
7, 15, 3, 5, 1.2, 0)`` line the reference carries beneath its DeepFlow call (:32), whose parameters are the defaults here.

Documented deviations: DeepFlow needs opencv-contrib and is not reproduced; the frames are resized with the
package's Pillow-exact Lanczos (K0) instead of cv2 ``INTER_LANCZOS4``; the gray conversion keeps the reference's quirk of
running ``COLOR_BGR2GRAY`` on an array whose channels were reversed first.

``FarnebackFlow`` is the batched form: the F + 1 frames of a video give F flows, and every frame's pyramid and polynomial
expansion is computed once (the reference redoes them for both frames of every pair).  Its output, f32 [F, H, W, 2] on the
device in (dx, dy) pixels with prev(y, x) ~ next(y + dy, x + dx), is what ``train_step`` consumes as [B, T, H, W, 2] and what
``utils.npy_io.save_motions`` writes as the reference's ``motion/{:06}.npy``.
"""
import numpy as np
import torch

from .. import ops
from ._device import host_tensor
from .._lib import check, lib, ptr, require_gpu, stream
from .resize import LanczosResize


class FarnebackFlow:
    """``FarnebackFlow((H, W))(gray)``: gray f32 [F + 1, H, W] (0 .. 255) on the GPU -> flow f32 [F, H, W, 2] on the GPU.
    Holds the level geometry and the workspace (grown to the largest F seen)."""

    def __init__(self, hw, pyr_scale=0.5, levels=7, winsize=15, iterations=3, poly_n=5, poly_sigma=1.2, device='cuda', flags=0):
        if flags != 0:
            raise ValueError("flags other than 0 (Gaussian window, initial flow) are not supported, got %r" % (flags,))
        if int(winsize) < 1 or int(winsize) % 2 == 0:
            raise ValueError("winsize must be odd, got %r" % (winsize,))
        if int(iterations) < 1:
            raise ValueError("iterations must be at least 1, got %r" % (iterations,))
        self.hw = (int(hw[0]), int(hw[1]))
        self.pyr_scale, self.levels, self.winsize = float(pyr_scale), int(levels), int(winsize)
        self.iterations, self.poly_n, self.poly_sigma = int(iterations), int(poly_n), float(poly_sigma)
        self.device = torch.device(device)
        self.geometry = ops.optflow_levels(self.hw[0], self.hw[1], self.pyr_scale, self.levels)     # [(h, w, ksz, sigma)]
        ops.optflow_poly_tables(self.poly_n, self.poly_sigma)                                       # refuses a bad poly_n / sigma
        self._work = None
        self._resize = {}

    def work_bytes(self, F):
        n = lib().cp360_optflow_work_bytes(int(F), self.hw[0], self.hw[1], self.pyr_scale, self.levels)
        if n == 0:
            raise ValueError("optical flow: unsupported geometry: %d pairs of %s" % (F, self.hw))
        return n

    def __call__(self, gray, out=None):
        require_gpu(gray, out)
        if gray.dtype != torch.float32 or gray.dim() != 3 or gray.shape[0] < 2 or tuple(gray.shape[1:]) != self.hw:
            raise ValueError("gray must be float32 [F + 1, %d, %d] with F >= 1, got %s %s"
                             % (self.hw + (gray.dtype, tuple(gray.shape))))
        gray = gray.contiguous()
        F, (H, W) = int(gray.shape[0]) - 1, self.hw
        if out is None:
            out = torch.empty((F, H, W, 2), dtype=torch.float32, device=gray.device)
        elif out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != (F, H, W, 2) \
                or out.device != gray.device:
            raise ValueError("out must be a contiguous float32 [%d, %d, %d, 2] on %s" % (F, H, W, gray.device))
        nbytes = self.work_bytes(F)
        if self._work is None or self._work.numel() * 4 < nbytes or self._work.device != gray.device:
            self._work = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=gray.device)
        check(lib().cp360_optflow_farneback(ptr(gray), F, H, W, self.pyr_scale, self.levels, self.winsize, self.iterations,
                                            self.poly_n, self.poly_sigma, 0, ptr(out), ptr(self._work),
                                            self._work.numel() * 4, stream()))
        return out

    def gray_from_frames(self, frames, res=None):
        """frames u8 [N, h, w, 3] as the video reader delivers them (host or device) -> gray f32 [N, H, W] on the device:
        the preamble of ``calcOpticalFlow`` (resize to ``res`` = (width, height), reversed channels, BGR2GRAY arithmetic)."""
        frames = host_tensor(frames)
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
            raise ValueError("frames must be uint8 [N, h, w, 3], got %s %s" % (frames.dtype, tuple(frames.shape)))
        res = (self.hw[1], self.hw[0]) if res is None else (int(res[0]), int(res[1]))
        if (res[1], res[0]) != self.hw:
            raise ValueError("res = (width, height) = %s does not match this flow's %d x %d" % (res, self.hw[0], self.hw[1]))
        frames = frames.to(self.device)
        in_hw = (int(frames.shape[1]), int(frames.shape[2]))
        if in_hw != self.hw:
            rs = self._resize.get(in_hw)
            if rs is None:
                rs = self._resize[in_hw] = LanczosResize(in_hw, self.hw, device=self.device)
            frames = rs(frames)
        return ops.optflow_gray(frames)

    def from_frames(self, frames, res=(960, 480)):
        """frames u8 [F + 1, h, w, 3] -> flow f32 [F, H, W, 2] on the device (``res`` = (width, height) must be this flow's)."""
        return self(self.gray_from_frames(frames, res))


def absflow_of(flow):
    """The reference's flow-intensity image (:34-37): magnitude, min-max normalised, values below mean - 1.5 std zeroed."""
    absflow = np.sqrt(flow[:, :, 0] ** 2 + flow[:, :, 1] ** 2)
    absflow = absflow - np.min(absflow)
    absflow = absflow / np.max(absflow)
    absflow[absflow < (np.mean(absflow) - 1.5 * np.std(absflow))] = 0
    return absflow


_FLOWS = {}


def calcOpticalFlow(prev_frame, cur_frame, res=(960, 480)):
    """
        Extract optical flow from two consecutive frames
        Args:
            prev_frame: previous frame (u8 [h, w, 3] numpy)
            cur_frame: current frame
            res: resolution: (width, height)
        Returns:
            absflow: Flow intensity image (f32 [height, width] numpy)
            flow: Optical flow (f32 [height, width, 2] numpy)
    """
    key = (int(res[1]), int(res[0]))
    ff = _FLOWS.get(key)
    if ff is None:
        ff = _FLOWS[key] = FarnebackFlow(key)
    frames = np.stack([np.asarray(prev_frame), np.asarray(cur_frame)])
    flow = ff.from_frames(frames, res)[0].cpu().numpy()
    return absflow_of(flow), flow
