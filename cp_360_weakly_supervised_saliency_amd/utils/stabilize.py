"""360-degree stabilisation of an equirectangular video (K11, csrc/stabilize.hip): the reference trains its temporal model on
"stationary videos (without camera motion)" only and leaves the rest to the user (README: "you might want to compensate camera
motion and apply 360 stabilization").  For an equirectangular frame a camera rotation is a remapping of the sphere: it is fitted
to the optical flow of every frame pair (K10 + ``ops.rotation_fit``) and removed by re-rendering the frames
(``ops.equirect_rotate``).  The definition is the package's own (DESIGN.md "K11").

``Stabilizer`` is the driver: ``rotations`` gives the per-pair and the cumulative camera rotations of F + 1 frames, ``stabilize``
the frames in the first frame's orientation - the input of ``SaliencyEngine`` and ``FarnebackFlow`` alike - and ``from_frames``
the flows of the stabilised video, which is what ``utils.npy_io.save_motions`` and ``train_step`` are fed for a moving camera.
Translation and parallax of the camera stay in that flow.  For a camera that travels, ``egomotion`` also fits the direction of
translation of every pair (K23, csrc/egomotion.hip) and ``independent_flow`` gives the part of the stabilised video's flow that
no static scene explains under that camera motion: the flow to feed ``save_motions`` / ``train_step`` then (DESIGN.md "K23").
"""
import numpy as np
import torch

from .. import ops
from ._device import TabWork, host_tensor, on_device
from .optical_flow import FarnebackFlow
from .shots import check_cuts, segments


def orthonormalise(M):
    """The rows of a float64 [3, 3] near-rotation by Gram-Schmidt (exact on I)."""
    r0 = M[0] / np.linalg.norm(M[0])
    r1 = M[1] - (M[1] @ r0) * r0
    r1 = r1 / np.linalg.norm(r1)
    r2 = M[2] - (M[2] @ r0) * r0 - (M[2] @ r1) * r1
    return np.stack([r0, r1, r2 / np.linalg.norm(r2)])


def compose(R, cuts=None):
    """R [F, 3, 3] (host) -> C float64 [F + 1, 3, 3]: C_0 = I, C_t+1 = R_t C_t, the chain in float64 and every C_t
    re-orthonormalised once on the way out: a scene direction p of frame 0's camera is seen at C_t p in frame t.
    ``cuts`` (``utils.shots``: the first frame of every new shot) restarts the chain: C_t = I exactly for t in cuts, and the
    R_t-1 of the pair that straddles the cut is not used; every shot is stabilised to its own first frame."""
    R = np.asarray(R, np.float64)
    starts = set(check_cuts(cuts, R.shape[0] + 1))
    C, out = np.eye(3), [np.eye(3)]
    for f in range(R.shape[0]):
        if f + 1 in starts:
            C = np.eye(3)
            out.append(np.eye(3))
            continue
        C = R[f] @ C
        out.append(orthonormalise(C))
    return np.stack(out)


class Stabilizer:
    """``Stabilizer((H, W))``: the rotation fit runs on flows of H x W (the frames are resized for it as ``FarnebackFlow`` does),
    the re-rendering at the frames' own resolution.  Holds the ``FarnebackFlow`` and the K11 workspaces."""

    def __init__(self, hw=(480, 960), device='cuda', iters=8, c_min_px=0.25):
        if int(iters) < 1 or not float(c_min_px) > 0.0:
            raise ValueError("iters must be at least 1 and c_min_px positive, got %r, %r" % (iters, c_min_px))
        self.hw = (int(hw[0]), int(hw[1]))
        self.device = torch.device(device)
        self.iters, self.c_min_px = int(iters), float(c_min_px)
        self.flow = FarnebackFlow(self.hw, device=device)
        self._fit_work = None
        self._ego_work = None
        self._tab_work = TabWork()
        self.diag = None                         # f64 [F, 4] of the last fit (device)

    def _frames(self, frames):
        frames = host_tensor(frames)
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or frames.shape[0] < 2:
            raise ValueError("frames must be uint8 [F + 1, h, w, 3] with F >= 1, got %s %s" % (frames.dtype, tuple(frames.shape)))
        return frames.to(self.device).contiguous()

    def rotations(self, frames, cuts=None):
        """frames u8 [F + 1, h, w, 3] -> (R f32 [F, 3, 3], C f32 [F + 1, 3, 3]) on the device.  ``cuts`` (``utils.shots``: the
        first frame of every new shot): the R of a pair that straddles a cut is I and its ``diag`` row zeros - the flow across
        a cut means nothing -, C restarts at I there, and every other R and C is what the shot's own frames give."""
        frames = self._frames(frames)
        cuts = check_cuts(cuts, int(frames.shape[0]))
        H, W = self.hw
        flows = self.flow.from_frames(frames, res=(W, H))
        F = int(flows.shape[0])
        self._fit_work = ops._stab_work(F, H, W, flows.device, self._fit_work)
        R, self.diag = ops.rotation_fit(flows, self.iters, self.c_min_px, work=self._fit_work)
        if cuts:
            pairs = torch.tensor([t - 1 for t in cuts], device=R.device)
            R[pairs] = torch.eye(3, dtype=R.dtype, device=R.device)
            self.diag[pairs] = 0.0
        C = compose(R.cpu().numpy(), cuts)
        return R, torch.from_numpy(C.astype(np.float32)).to(self.device)

    def stabilize(self, frames, cuts=None):
        """frames u8 [F + 1, h, w, 3] -> (the frames in frame 0's orientation, S_t(p) = frame_t(C_t p), u8 on the device; C).
        Frame 0 is copied.  With ``cuts`` every shot is brought to the orientation of its own first frame, which is copied."""
        frames = self._frames(frames)
        _, C = self.rotations(frames, cuts)
        out = torch.empty_like(frames)
        for lo, hi in segments(cuts, int(frames.shape[0])):
            out[lo].copy_(frames[lo])
            if hi - lo > 1:
                self.render(frames[lo + 1:hi], C[lo + 1:hi], out=out[lo + 1:hi])
        return out, C

    def render(self, frames, C, out=None):
        """frames u8 [N, h, w, 3] under the rotations C f32 [N, 3, 3] (for instance ``rotations``' C after a smoothing of the
        caller's): out[n](p) = frames[n](C[n] p), at the frames' own resolution, on the device."""
        frames, C = on_device(frames, self.device), on_device(C, self.device, torch.float32)
        return ops.equirect_rotate(frames, C, out=out, work=self._tab_work(frames))

    def from_frames(self, frames):
        """frames u8 [F + 1, h, w, 3] -> the flows f32 [F, H, W, 2] of the stabilised video, on the device.  It takes no ``cuts``:
        a flow across a cut has no meaning and must not reach ``npy_io.save_motions`` / ``train_step``.  For a video with cuts
        call it on every shot of two frames or more: ``for lo, hi in utils.shots.segments(cuts, n): if hi - lo >= 2: ...
        from_frames(frames[lo:hi])``."""
        H, W = self.hw
        return self.flow.from_frames(self.stabilize(frames)[0], res=(W, H))

    def _ego(self, flows, cuts, t_min_px, min_share):
        """K23a on the flows, from K11's fit of them; pairs that straddle a cut get R = I, e = 0 and a diag row of zeros."""
        F, (H, W) = int(flows.shape[0]), self.hw
        self._ego_work = ops._ego_work(F, H, W, flows.device, self._ego_work)
        R, e, diag = ops.egomotion_fit(flows, None, self.iters, self.c_min_px, t_min_px, min_share, work=self._ego_work)
        if cuts:
            pairs = torch.tensor([t - 1 for t in cuts], device=R.device)
            R[pairs] = torch.eye(3, dtype=R.dtype, device=R.device)
            e[pairs] = 0.0
            diag[pairs] = 0.0
        return R, e, diag

    def egomotion(self, frames, cuts=None, t_min_px=0.25, min_share=0.25):
        """frames u8 [F + 1, h, w, 3] -> (R f32 [F, 3, 3], e f32 [F, 3], diag f64 [F, 8]) on the device: K10 at ``hw``, K11, then
        K23a (``ops.egomotion_fit``).  e is the unit direction of the camera's translation in the pair's own camera frame (frame
        t's axes), or 0 where the pair shows no translation; its length is not observable.  A pair that straddles a cut has
        R = I, e = 0 and a diag row of zeros, as ``rotations`` treats it."""
        frames = self._frames(frames)
        cuts = check_cuts(cuts, int(frames.shape[0]))
        H, W = self.hw
        flows = self.flow.from_frames(frames, res=(W, H))
        return self._ego(flows, cuts, t_min_px, min_share)

    def independent_flow(self, frames, cuts=None, t_min_px=0.25, min_share=0.25):
        """frames u8 [F + 1, h, w, 3] -> (res f32 [F, H, W, 2], e f32 [F, 3], diag f64 [F, 8]) on the device: the frames are
        stabilised as ``stabilize`` does, K10 runs on the result, K23a fits what rotation is left and the direction of translation
        to those flows and K23b removes what they explain.  res is what ``npy_io.save_motions`` and ``train_step`` are fed for a
        travelling camera.  e is in each pair's own stabilised camera frame: the axes of the first frame of its shot.  With
        ``cuts`` the pair that straddles a cut has e = 0 and its res is the plain flow across the cut, which means nothing: keep
        it out of training as ``from_frames`` says.  One host synchronisation, that of ``rotations``."""
        frames = self._frames(frames)
        cuts = check_cuts(cuts, int(frames.shape[0]))
        H, W = self.hw
        flows = self.flow.from_frames(self.stabilize(frames, cuts)[0], res=(W, H))
        R, e, diag = self._ego(flows, cuts, t_min_px, min_share)
        return ops.egomotion_residual(flows, R, e, work=self._ego_work), e, diag
