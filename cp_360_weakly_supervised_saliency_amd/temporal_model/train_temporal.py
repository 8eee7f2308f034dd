"""Weakly supervised ConvLSTM training from optical flow: the reference's temporal_model/train_temporal.py:24-193 with the
reference's names.  The window's cell updates, saliency maps and their backward pass run in libcp360.so
(``model.clstm_train``); so do the flow resize and the flow loss with its backward pass (``resize_flow``,
``device_flow_losses``: csrc/flow_loss.hip), whose gradient reaches the window's kernels through autograd.

Behaviour kept from the reference:
  * min / max normalisation over the WHOLE batch - all clips, all frames (:74-82), not per window as in test_temporal;
  * every flow the loss reads is resized with cv2.resize(INTER_CUBIC) to (2 flow_h, flow_h) (:112-113) - OpenCV's generic
    float path restated in HIP; cv2 copies at equal sizes - and multiplied by ``fscale = flow_h / W`` of the ORIGINAL flow
    (:110-111): it divides by the flow's WIDTH, so flow stored at the loss resolution [flow_h, 2 flow_h] is multiplied by 0.5;
  * ``upsample(mode='bilinear')`` and ``grid_sample`` with the align_corners defaults of torch >= 1.3 (False), while
    ``generate_meshgrid`` uses the (h - 1) convention;
  * the reference scales ``flow_buff`` entries in place (:128-129); each entry is used once, so that is harmless - here the
    scaled flow is a new tensor.
Flow of any [H, W] is accepted; only the tmp_loss_len flows the loss reads are copied to the device.  ``flow_losses`` is the torch
restatement of the loss at the loss resolution (flow already [flow_h, 2 flow_h]): the reference for the HIP loss, and the path
``train_step`` takes for a criterion other than the reference's sum-MSE.
"""
import os
import time
import types

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from .._lib import PRECISIONS
from ..model.clstm_train import trainer_of, window_maps


def generate_meshgrid(flow):
    """flow [N, h, w, ...] -> [N, 2, h, w] f32: (x, y) in [-1, 1] on the (size - 1) grid (:24-30), on flow's device."""
    h = flow.size(1)
    w = flow.size(2)
    y = torch.arange(0, h).unsqueeze(1).repeat(1, w) / (h - 1) * 2 - 1
    x = torch.arange(0, w).unsqueeze(0).repeat(h, 1) / (w - 1) * 2 - 1
    mesh_grid = torch.stack([x, y], 0).unsqueeze(0).repeat(flow.size(0), 1, 1, 1).to(flow.device)
    return mesh_grid.float()


def _stack(items):
    return items if torch.is_tensor(items) else torch.stack(list(items), 1)


def normalize_batch(seq):
    """seq [B, T, 6, C, w, w] -> (seq - min) / max(seq - min), both over the whole batch (:74-85)."""
    min_seq = seq.min()
    max0min_seq = (seq - min_seq).max()
    return (seq - min_seq) / max0min_seq


def check_flow(flow, flow_h):
    """flow [B, T, H_f, W_f, 2]: only the loss resolution (flow_h, 2 flow_h) is accepted (cv2.resize would be the identity)."""
    if flow.dim() != 5 or flow.shape[-1] != 2:
        raise ValueError("flow must be [B, T, H, W, 2], got %s" % (tuple(flow.shape),))
    if tuple(flow.shape[2:4]) != (flow_h, 2 * flow_h):
        raise ValueError("flow must already be at the loss resolution %dx%d (the reference's cv2.resize INTER_CUBIC to "
                         "(2 flow_h, flow_h) is not reproduced), got %dx%d" % (flow_h, 2 * flow_h, flow.shape[2], flow.shape[3]))


def flow_losses(maps, flow, cfg, tmp_loss_len=3, criterion=None):
    """The three loss terms of :115-167.  maps [B, tmp_loss_len + 1, 2w, 4w]: the saliency maps of steps
    seq_len - tmp_loss_len - 1 .. seq_len - 1; flow [B, T, flow_h, 2 flow_h, 2].  Returns (loss_sm, loss_temp, loss_mask)."""
    criterion = criterion or nn.MSELoss(reduction='sum')
    B = maps.shape[0]
    flow_h = cfg.flow_h
    check_flow(flow, flow_h)
    first = cfg.seq_len - tmp_loss_len - 1
    fscale = flow_h / float(flow.size(3))                      # flow[idx].size(2) of a [B, H, W, 2] tensor: the width
    size = (flow.size(2), flow.size(3))
    mesh_grid = generate_meshgrid(flow[0, 0].unsqueeze(0)).permute(0, 2, 3, 1)
    loss_sm = loss_temp = loss_mask = None
    for i_b in range(B):
        for fidx in range(tmp_loss_len):
            tmp_flow = (fscale * flow[i_b, first + fidx]).unsqueeze(0)
            motion_mask = torch.sqrt(tmp_flow[0, :, :, 0] ** 2 + tmp_flow[0, :, :, 1] ** 2) < cfg.mm_th
            tmp_feat = F.interpolate(maps[i_b, fidx][None, None], size=size, mode='bilinear', align_corners=False)
            tmp_feat_next = F.interpolate(maps[i_b, fidx + 1][None, None], size=size, mode='bilinear', align_corners=False)
            tmp_flow = torch.stack([tmp_flow[..., 0] / tmp_feat.size()[3] * 2, tmp_flow[..., 1] / tmp_feat.size()[2] * 2], -1)
            tmp_grid = tmp_flow + mesh_grid
            warp_prediction = F.grid_sample(tmp_feat, tmp_grid, align_corners=False).detach()
            tmp_feat_val = tmp_feat.detach()
            tmp_feat_val_mask = tmp_feat_next.detach().clone()
            tmp_feat_val_mask[:, :, motion_mask] = 0
            terms = (criterion(tmp_feat_next, warp_prediction), criterion(tmp_feat_next, tmp_feat_val),
                     criterion(tmp_feat_next, tmp_feat_val_mask))
            if loss_sm is None:
                loss_sm, loss_temp, loss_mask = terms
            else:
                loss_sm, loss_temp, loss_mask = loss_sm + terms[0], loss_temp + terms[1], loss_mask + terms[2]
    return loss_sm, loss_temp, loss_mask


def resize_flow(flow, flow_h):
    """The reference's :110-113 on the device: flow f32 [..., H, W, 2] (a GPU tensor) -> cv2.resize(flow, (2 flow_h, flow_h),
    INTER_CUBIC) * (flow_h / W), f32 [..., flow_h, 2 flow_h, 2].  OpenCV's generic float path (csrc/flow_loss.hip); cv2 itself
    is not pinned by the tests, which check a restatement of that path (as for the cv2.remap of SURVEY a2): an IPP build of
    OpenCV may differ in the last bits."""
    if flow.dim() < 3 or flow.shape[-1] != 2:
        raise ValueError("flow must be [..., H, W, 2], got %s" % (tuple(flow.shape),))
    fscale = flow_h / float(flow.shape[-2])
    return ops.flow_resize(flow.contiguous(), int(flow_h), 2 * int(flow_h), fscale)


class DeviceFlowLoss(torch.autograd.Function):
    """(loss_sm, loss_temp, loss_mask) = DeviceFlowLoss.apply(maps, flow_scaled, mm_th, events): the three sum-MSE terms of
    ``flow_losses`` over all B x tmp_loss_len pairs in HIP (cp360_flow_loss_forward / _backward).  The gradient reaches maps only
    (map fidx + 1 of each pair); the backward recomputes the residuals from the maps and the flow."""

    @staticmethod
    def forward(ctx, maps, flow_scaled, mm_th, events):
        maps = maps.detach().float().contiguous()
        flow_scaled = flow_scaled.detach().contiguous()
        _mark(events, 'loss')
        loss = ops.flow_loss_forward(maps, flow_scaled, mm_th)
        _mark(events, 'loss_end')
        ctx.save_for_backward(maps, flow_scaled)
        ctx.mm_th, ctx.events = mm_th, events
        return loss[0], loss[1], loss[2]

    @staticmethod
    def backward(ctx, g_sm, g_t, g_m):
        maps, flow_scaled = ctx.saved_tensors
        z = lambda g: torch.zeros((), dtype=torch.float32, device=maps.device) if g is None else g.float().reshape(())
        _mark(ctx.events, 'loss_bwd')
        dmaps = ops.flow_loss_backward(maps, flow_scaled, torch.stack([z(g_sm), z(g_t), z(g_m)]).contiguous(), ctx.mm_th)
        _mark(ctx.events, 'loss_bwd_end')
        return dmaps, None, None, None


def _mark(events, name):
    """Measurement hook (tools/train_bench.py, never set in training): (phase, HIP event) pairs on the launch stream."""
    if events is not None:
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        events.append((name, e))


def device_flow_losses(maps, flow_scaled, cfg, tmp_loss_len=3, events=None):
    """``flow_losses`` in HIP: maps f32 [B, tmp_loss_len + 1, 2w, 4w] (the saliency maps of steps seq_len - tmp_loss_len - 1
    .. seq_len - 1, on the GPU), flow_scaled f32 [B, tmp_loss_len, H, W, 2] = ``resize_flow`` of the flows of steps
    seq_len - tmp_loss_len - 1 .. seq_len - 2.  Returns (loss_sm, loss_temp, loss_mask), differentiable with respect to maps."""
    if maps.dim() != 4 or maps.shape[1] != tmp_loss_len + 1:
        raise ValueError("maps must be [B, tmp_loss_len + 1 = %d, 2w, 4w], got %s" % (tmp_loss_len + 1, tuple(maps.shape)))
    if flow_scaled.dim() != 5 or flow_scaled.shape[1] != tmp_loss_len or flow_scaled.shape[0] != maps.shape[0]:
        raise ValueError("flow_scaled must be [B, tmp_loss_len = %d, H, W, 2], got %s" % (tmp_loss_len, tuple(flow_scaled.shape)))
    return DeviceFlowLoss.apply(maps, flow_scaled, float(cfg.mm_th), events)


def _is_sum_mse(criterion):
    return criterion is None or (type(criterion) is nn.MSELoss and criterion.reduction == 'sum')


def _loss_flows(flow, T, first, tmp_loss_len, dev):
    """The tmp_loss_len flows the loss reads as f32 [B, tmp_loss_len, H, W, 2] on dev: only those are copied, each from a
    contiguous piece of the host tensors (a clip's run of frames, or one frame's batch)."""
    sel = range(first, first + tmp_loss_len)
    if torch.is_tensor(flow):
        if flow.dim() != 5 or flow.shape[-1] != 2 or flow.shape[1] != T:
            raise ValueError("flow must be [B, T = %d, H, W, 2], got %s" % (T, tuple(flow.shape)))
        B, _, H, W, _ = flow.shape
        out = torch.empty((B, tmp_loss_len, H, W, 2), dtype=torch.float32, device=dev)
        for b in range(B):
            out[b].copy_(flow[b, first:first + tmp_loss_len])
        return out
    flow = list(flow)
    if len(flow) != T:
        raise ValueError("flow must hold seq_len = %d frames" % T)
    parts = [torch.as_tensor(flow[t]) for t in sel]
    if any(f.dim() != 4 or f.shape[-1] != 2 or f.shape != parts[0].shape for f in parts):
        raise ValueError("flow must be T tensors [B, H, W, 2] of one shape")
    out = torch.empty((parts[0].shape[0], tmp_loss_len) + tuple(parts[0].shape[1:]), dtype=torch.float32, device=dev)
    for l, f in enumerate(parts):
        out[:, l].copy_(f)
    return out


def train_step(cell, seq, flow, optimizer, cfg, tmp_loss_len=3, criterion=None):
    """One iteration of train() on one batch: seq = T tensors [B, 6, C, w, w] (or [B, T, 6, C, w, w]), flow = T tensors
    [B, H, W, 2] (or [B, T, H, W, 2]) of any H x W.  Normalise, forward, resize the flows the loss reads, loss,
    ``optimizer.zero_grad(); loss.backward(); optimizer.step()``.  Returns the three loss terms (loss_sm, loss_temp, loss_mask)
    as detached tensors.  The loss runs in HIP for the reference's criterion (None or ``nn.MSELoss(reduction='sum')``); any
    other criterion goes through ``flow_losses`` on the same resized flow."""
    dev = cell.Conv1.weight.device
    seq = _stack(seq).to(dev, torch.float32)
    if seq.dim() != 6 or seq.shape[2] != 6:
        raise ValueError("seq must be T tensors [B, 6, C, w, w]")
    B, T, _, C, w, _ = seq.shape
    if T != cfg.seq_len:
        raise ValueError("seq / flow must hold seq_len = %d frames" % cfg.seq_len)
    if not 0 <= cfg.seq_len - tmp_loss_len - 1:
        raise ValueError("tmp_loss_len must be < seq_len")
    first = cfg.seq_len - tmp_loss_len - 1
    events = trainer_of(cell).events
    _mark(events, 'resize')
    flow = _loss_flows(flow, T, first, tmp_loss_len, dev)
    if flow.shape[0] != B:
        raise ValueError("flow must hold the batch's %d clips" % B)
    scaled = resize_flow(flow, cfg.flow_h)                                          # [B, tmp_loss_len, flow_h, 2 flow_h, 2]
    _mark(events, 'resize_end')
    frames = normalize_batch(seq).permute(0, 1, 2, 4, 5, 3).reshape(B, T, 6 * w * w, C).contiguous()
    maps = window_maps(cell, frames, range(first, T))
    if _is_sum_mse(criterion):
        loss_sm, loss_temp, loss_mask = device_flow_losses(maps, scaled, cfg, tmp_loss_len, events)
    else:
        # flow_losses multiplies by flow_h / (2 flow_h) = 0.5 itself: 2 * scaled undoes that exactly
        sub = types.SimpleNamespace(flow_h=cfg.flow_h, mm_th=cfg.mm_th, seq_len=tmp_loss_len + 1)
        loss_sm, loss_temp, loss_mask = flow_losses(maps, 2.0 * scaled, sub, tmp_loss_len, criterion)
    loss = cfg.l_s * loss_sm + cfg.l_t * loss_temp + cfg.l_m * loss_mask
    optimizer.zero_grad()
    loss.backward()
    optimizer.step()
    return loss_sm.detach(), loss_temp.detach(), loss_mask.detach()


class FusedAdam(torch.optim.Adam):
    """``torch.optim.Adam`` over ``cell.parameters()`` whose step runs in libcp360.so (csrc/adam.hip): one pass over each
    parameter, its gradient and its two moments that also writes the new weights into the packs the cell's training plan
    holds (the forward convolutions' and the dgrad operands), so the next ``train_step`` repacks nothing.  Every other holder
    of packed weights (``ConvLSTMCell.plans()``, the Winograd packs, a stage context) sees the parameters' version counters
    move and repacks as after any optimizer step.

    State and param groups are torch.optim.Adam's (``step``, ``exp_avg``, ``exp_avg_sq``), so ``state_dict()`` /
    ``load_state_dict()`` interchange with it in both directions; ``zero_grad``, ``param_groups`` and LR schedulers are
    inherited.  amsgrad, maximize, capturable, differentiable, a closure and sparse gradients are refused (ValueError); a
    parameter whose ``.grad`` is None is skipped.  GPU only, f32 parameters."""

    def __init__(self, cell, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, maximize=False,
                 capturable=False):
        _refuse_adam_variants(dict(amsgrad=amsgrad, maximize=maximize, capturable=capturable))
        super().__init__(cell.parameters(), lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        self.cell = cell

    def _cell_packs(self):
        """(trainer, {id(filter): pack arguments of ops.adam_step_conv}) when the cell's training plan is current, else
        (None, {}): stale or absent packs are left to the lazy rule."""
        cell = self.cell
        tr = cell.__dict__.get('_trainer')
        if tr is None or tr.cell is not cell or not tr.current():
            return None, {}
        plan = tr.plans()
        dt = PRECISIONS[cell.precision]
        packs = {}
        for w, conv, dg in ((cell.Conv1.weight, plan['c1'], plan['d1']), (cell.Conv2.weight, plan['c2'], plan['d2']),
                            (cell.Gates.weight, plan['g'], plan['dg'])):
            packs[id(w)] = dict(dtype=dt, fwd_tap_major=conv._packed.get(0), fwd_chan_major=conv._packed.get(1),
                                dgrad_packed=dg.packed, ci0=dg.ci0, n_dgrad=dg.n)
        return tr, packs

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise ValueError("FusedAdam.step takes no closure")
        tr, packs = self._cell_packs()
        scalar = torch.float64 if torch.get_default_dtype() == torch.float64 else torch.float32      # as torch.optim.Adam
        for group in self.param_groups:
            _refuse_adam_variants(group)
            for p in group['params']:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise ValueError("FusedAdam does not take sparse gradients")
                ops.require_gpu(p)
                state = self.state[p]
                if len(state) == 0:
                    state['step'] = torch.tensor(0.0, dtype=scalar)
                    state['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                state['step'] += 1
                hyper = dict(lr=float(group['lr']), betas=group['betas'], eps=group['eps'],
                             weight_decay=group['weight_decay'], step=int(state['step'].item()))
                args = (p.detach(), p.grad.contiguous(), state['exp_avg'], state['exp_avg_sq'])
                if p.dim() == 4 and tuple(p.shape[2:]) == (3, 3) and p.shape[1] % 4 == 0:
                    ops.adam_step_conv(*args, **hyper, **packs.get(id(p), {}))
                else:
                    ops.adam_step(*args, **hyper)
                torch.autograd.graph.increment_version(p)
        if tr is not None:
            tr.adopt()
        return None


def _refuse_adam_variants(group):
    for key in ('amsgrad', 'maximize', 'capturable', 'differentiable'):
        if group.get(key):
            raise ValueError("FusedAdam is torch.optim.Adam with %s=False only" % key)


def train(train_loader, model, criterion, optimizer, epoch, out_model_path, init_iter, cfg, tmp_loss_len=3):
    """Train the temporal model for one epoch (:33-193): checkpoints 'CLSTM_[epoch]_[iteration].pth' every save_freq."""
    assert cfg.use_gpu
    model.train()
    batch_time = 0.0
    running_loss = 0.0
    for i, (seq, flow, _, _) in enumerate(train_loader):
        ttime = time.time()
        i += init_iter
        if i > len(train_loader) + 1:
            break
        loss_sm, loss_temp, loss_mask = train_step(model, seq, flow, optimizer, cfg, tmp_loss_len, criterion)
        loss = cfg.l_s * loss_sm + cfg.l_t * loss_temp + cfg.l_m * loss_mask
        if i % cfg.summary_freq == (cfg.summary_freq - 1):
            print("Smooth loss: {0:.3f}, Tmp loss: {1:.3f}, MMask loss: {2:.3f}".format(cfg.l_s * loss_sm.item(),
                                                                                        cfg.l_t * loss_temp.item(),
                                                                                        cfg.l_m * loss_mask.item()))
        batch_time += time.time() - ttime
        running_loss += loss.item()
        if i % cfg.summary_freq == (cfg.summary_freq - 1):
            print("Epoch: [{}][{}/{}]\t Loss (avg.): {:.3f}\t Batch Time (avg.):{:.3f}".format(epoch,
                  i + 1, len(train_loader), running_loss / cfg.summary_freq, batch_time / cfg.summary_freq))
            batch_time = 0.0
            running_loss = 0.0
        if i % cfg.save_freq == (cfg.save_freq - 1):
            print(os.path.join(out_model_path, 'CLSTM_{0:02}_{1:06}.pth'.format(epoch, i)))
            torch.save(model.state_dict(), os.path.join(out_model_path, 'CLSTM_{0:02}_{1:06}.pth'.format(epoch, i)))
