"""The windows of TWO independent batches in one run of the T cell updates (cp360_clstm_window_multi, csrc/ctx.hip), beside
``ClipRunner`` (test_temporal.py in this package), whose cell, projection and shapes it shares: at 2B clips every Winograd GEMM
launch streams its filters from HBM once for both batches, and every GEMM row is still the arithmetic of ``ClipRunner.run``.
"""
import torch

from .. import stage_ctx


class PairRunner:
    def __init__(self, runner):
        self.runner = runner                               # the ClipRunner of ONE batch
        self.h = None                                      # the two batches' final hidden states, f32 [6B, w, w, H] each
        self.minmax = None                                 # f32 [2B, 2]: batch a's window min / max rows, then batch b's

    def _stage(self):
        cell = self.runner.cell
        stage = cell.__dict__.get('_stage')
        if stage is None:
            stage = cell.__dict__['_stage'] = stage_ctx.ClstmStage(cell)
        return stage

    def can_pair(self):
        """True when ``run`` gives, for each of the two batches, the bits of ``ClipRunner.run``: see ClstmStage.can_pair."""
        r = self.runner
        return stage_ctx.USE_CTX and r.cell.input_size == r.cell.hidden_size and self._stage().can_pair(r.B, r.w)

    def run(self, cam_a, cam_b, return_all_steps=False):
        """cam_a / cam_b: each as ``ClipRunner.run``'s dense ``cam``.  Returns the two batches' maps, each what
        ``ClipRunner.run`` returns for it."""
        r = self.runner
        B, T = r.B, r.T
        if self.h is None:
            self.h = [torch.empty_like(r.h_f32) for _ in range(2)]
            self.minmax = torch.empty((2 * B, 2), dtype=torch.float32, device=r.h_f32.device)
        h_alls = None
        if return_all_steps:
            h_alls = [torch.empty((T,) + tuple(r.h_f32.shape), dtype=torch.float32, device=r.h_f32.device) for _ in range(2)]
        self._stage().window_multi([cam_a, cam_b], B, T, r.w, self.h, self.minmax, h_alls=h_alls)
        # cube -> equi batch by batch: the launches of two ``ClipRunner.run`` calls
        if return_all_steps:
            return tuple(torch.stack([r.c2e.saliency(h[t], layout='nhwc') for t in range(T)], dim=1) for h in h_alls)
        return tuple(r.c2e.saliency(h, layout='nhwc') for h in self.h)
