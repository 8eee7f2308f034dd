"""Training of ``ConvLSTMCell`` (the reference's temporal_model/train_temporal.py:87-170): one window of T cell updates as a
``torch.autograd.Function`` whose forward and backward run in libcp360.so ("K5t", csrc/clstm_train.hip).

Forward, per step t (the cell of model/clstm.py:54-80):  xh_t = [x_t | h_{t-1}]  ->  a1_t = ReLU(Conv1(CubePad(xh_t)))  ->
a2_t = ReLU(Conv2(CubePad(a1_t)))  ->  Gates(CubePad(a2_t)) raw f32 sums  ->  cp360_train_gates (c_t, h_t and the four
activated gates).  Conv1 / Conv2 / Gates run on the direct kernels of inference (``ops.Conv``, cp360_conv_forward).  Kept for
the backward pass: xh_t, a1_t, a2_t (compute dtype), the gates and c_t (f32), h_t (f32) and the argmax channel of each map.

Backward (BPTT), t = T-1 .. 0:  dh_t += d map_t (cp360_train_saliency_backward)  ->  gates backward -> dG_t  ->  dgrad Gates,
CubePad adjoint, ReLU mask of a2_t -> dY2_t  ->  dgrad Conv2, mask a1_t -> dY1_t  ->  dgrad of Conv1's hidden half -> dh_{t-1}.
Then ONE wgrad launch per convolution over all T steps (dW and db).  The gradients come back to autograd, so they land in
``.grad`` of Conv1 / Conv2 / Gates and any torch.optim optimizer applies them.
"""
import numpy as np
import torch

from .. import ops
from .._lib import PRECISIONS
from ..utils.cube_to_equi import Cube2Equi
from .clstm import _stamp

TRAIN_PRECISIONS = ('fp32', 'bf16')
TRAIN_FACE = 7          # cube 224 after ResNet-50 (the reference's training configuration)


class ClstmTraining:
    """Device state of one cell's training: the forward convolutions, the dgrad packs and the inverse tables.  Packs are made
    again whenever a parameter's ``_version`` changes (an optimizer step) - the rule of ``ConvLSTMCell.plans()`` - unless the
    optimizer wrote them itself (``adopt``: temporal_model.train_temporal.FusedAdam)."""

    def __init__(self, cell):
        if cell.precision not in TRAIN_PRECISIONS:
            raise ValueError("training runs in precision 'fp32' or 'bf16' (got %r)" % cell.precision)
        if cell.input_size != cell.hidden_size:
            raise ValueError("training needs input_size == hidden_size (hidden = cell = frame 0, train_temporal.py:87-90)")
        self.cell = cell
        self._plan, self._stamp = None, None
        self._tables = {}
        # measurement hook (tools/train_bench.py, never set in training): a list that receives (phase, HIP event) pairs of the
        # launch stream at the phase boundaries 'forward', 'forward_end', 'bptt', 'wgrad', 'wgrad_end'
        self.events = None

    def _mark(self, name):
        if self.events is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self.events.append((name, e))

    def plans(self):
        cell = self.cell
        stamp = _stamp(cell, (cell.precision,))
        if self._plan is None or stamp != self._stamp:
            dt = PRECISIONS[cell.precision]
            dev = cell.Conv1.weight.device
            ops.require_gpu(cell.Conv1.weight)
            cin, hc = cell.input_size, cell.hidden_size
            p = {
                'c1': ops.Conv(cell.Conv1.weight, None, cell.Conv1.bias, 1, 1, True, dt, dev),
                'c2': ops.Conv(cell.Conv2.weight, None, cell.Conv2.bias, 1, 1, True, dt, dev),
                'g': ops.Conv(cell.Gates.weight, None, None, 1, 1, False, dt, dev),
                'gbias': cell.Gates.bias.detach().to(device=dev, dtype=torch.float32).contiguous(),
                'd1': ops.DgradPack(cell.Conv1.weight, cin, hc, dt),          # hidden half only: the frames need no gradient
                'd2': ops.DgradPack(cell.Conv2.weight, 0, 4 * hc, dt),
                'dg': ops.DgradPack(cell.Gates.weight, 0, 4 * hc, dt),
            }
            for k, name in (('c1', 'clstm.Conv1'), ('c2', 'clstm.Conv2'), ('g', 'clstm.Gates')):
                p[k].tag = name
            self._plan, self._stamp = p, stamp
        return self._plan

    def current(self):
        """True when the packs of ``plans()`` exist and belong to the parameters as they are now (no repack is pending)."""
        return self._plan is not None and self._stamp == _stamp(self.cell, (self.cell.precision,))

    def adopt(self):
        """For a writer that has brought the packs up to date with the parameters itself (``FusedAdam.step`` writes the new
        weights into them and bumps the parameters' versions): take the parameters' new stamp, so that ``plans()`` keeps
        returning the same objects without a pack launch.  The bias copies alias their parameters when those are f32,
        contiguous and on the device; any that do not are refreshed here."""
        if self._plan is None:
            return
        cell, p = self.cell, self._plan
        for copy, b in ((p['c1'].bias, cell.Conv1.bias), (p['c2'].bias, cell.Conv2.bias), (p['gbias'], cell.Gates.bias)):
            if copy.data_ptr() != b.data_ptr():
                copy.copy_(b.detach())
        self._stamp = _stamp(cell, (cell.precision,))

    def tables(self, w, dev):
        key = (w, str(dev))
        t = self._tables.get(key)
        if t is None:
            c2e = Cube2Equi(w, device=dev)
            fm, pc = c2e._tables()
            eo, ee = ops.c2e_inverse(fm.cpu().numpy(), pc.cpu().numpy(), w)
            po, pe = ops.cubepad_inverse(w)
            tab = ops.cubepad_table(w, 1)
            d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            t = dict(fm=fm, pc=pc, c2e_off=d(eo), c2e_ent=d(ee), pad_off=d(po), pad_ent=d(pe), pad_tab=d(tab))
            self._tables[key] = t
        return t

    # ------------------------------------------------------------------ forward
    def forward(self, frames, map_steps):
        """frames f32 [B, T, 6 w w, C] (normalised) -> maps f32 [B, len(map_steps), 2w, 4w] and the saved tensors."""
        ops.require_gpu(frames)
        cell = self.cell
        B, T, P, cin = frames.shape
        w = int(round((P / 6) ** 0.5))
        if 6 * w * w != P or cin != cell.input_size:
            raise ValueError("frames must be [B, T, 6 w^2, %d]" % cell.input_size)
        if w != TRAIN_FACE:
            raise ValueError("training is built for 7x7 faces (cube 224), got %dx%d" % (w, w))
        if frames.dtype != torch.float32:
            raise ValueError("frames must be f32")
        map_steps = tuple(int(s) for s in map_steps)
        if not map_steps or any(s < 0 or s >= T for s in map_steps) or len(set(map_steps)) != len(map_steps):
            raise ValueError("map_steps must be distinct steps in [0, %d)" % T)
        p = self.plans()
        tb = self.tables(w, frames.device)
        self._mark('forward')
        dt = PRECISIONS[cell.precision]
        dev, hc, n6 = frames.device, cell.hidden_size, 6 * B
        M = n6 * w * w
        fr = frames.view(B, T, 6, w, w, cin)
        xh = torch.empty((T + 1, n6, w, w, cin + hc), dtype=dt, device=dev)     # [T]: the last step's hidden (unused)
        for t in range(T):
            xh[t, ..., :cin].copy_(fr[:, t].reshape(n6, w, w, cin))
        xh[0, ..., cin:].copy_(fr[:, 0].reshape(n6, w, w, cin))                # hidden = frame 0 (:87-90)
        cs = torch.empty((T + 1, M, hc), dtype=torch.float32, device=dev)        # cs[t + 1] = c_t, cs[0] = frame 0
        cs[0].copy_(fr[:, 0].reshape(M, cin))
        a1 = torch.empty((T, n6, w, w, 4 * hc), dtype=dt, device=dev)
        a2 = torch.empty_like(a1)
        acts = torch.empty((T, M, 4 * hc), dtype=torch.float32, device=dev)
        hs = torch.empty((T, n6, w, w, hc), dtype=torch.float32, device=dev)
        for t in range(T):
            p['c1'](xh[t], out=a1[t])
            p['c2'](a1[t], out=a2[t])
            part, splits = p['g'](a2[t], raw_f32=True, slab_rows=False)
            ops.train_gates(part, splits, p['gbias'], cs[t], cs[t + 1], xh[t + 1], cin, hs[t], acts[t], M, hc)
        n = len(map_steps)
        maps = torch.empty((n, B, 2 * w, 4 * w), dtype=torch.float32, device=dev)
        amax = torch.empty((n, B, 2 * w, 4 * w), dtype=torch.int32, device=dev)
        for j, s in enumerate(map_steps):
            ops.saliency_forward(hs[s], tb['fm'], tb['pc'], maps[j], amax[j])
        self._mark('forward_end')
        saved = dict(xh=xh, a1=a1, a2=a2, acts=acts, cs=cs, hs=hs, amax=amax, map_steps=map_steps, B=B, T=T, w=w)
        return maps.permute(1, 0, 2, 3).contiguous(), saved

    # ------------------------------------------------------------------ backward
    def backward(self, saved, dmaps):
        """dmaps f32 [B, n, 2w, 4w] -> (dW1, db1, dW2, db2, dWg, dbg) f32."""
        cell = self.cell
        p = self.plans()
        B, T, w = saved['B'], saved['T'], saved['w']
        dev = dmaps.device
        tb = self.tables(w, dev)
        dt = PRECISIONS[cell.precision]
        cin, hc, n6 = cell.input_size, cell.hidden_size, 6 * B
        M = n6 * w * w
        xh, a1, a2, acts, cs, amax = (saved[k] for k in ('xh', 'a1', 'a2', 'acts', 'cs', 'amax'))
        self._mark('bptt')
        dm = dmaps.float().permute(1, 0, 2, 3).contiguous()
        dh = torch.zeros((n6, w, w, hc), dtype=torch.float32, device=dev)
        dc = torch.zeros((M, hc), dtype=torch.float32, device=dev)
        dG = torch.empty((T, n6, w, w, 4 * hc), dtype=dt, device=dev)
        dY2 = torch.empty_like(dG)
        dY1 = torch.empty_like(dG)
        pad4 = torch.empty((n6, w + 2, w + 2, 4 * hc), dtype=torch.float32, device=dev)
        pad1 = torch.empty((n6, w + 2, w + 2, hc), dtype=torch.float32, device=dev)
        where = {s: j for j, s in enumerate(saved['map_steps'])}
        for t in range(T - 1, -1, -1):
            if t in where:
                j = where[t]
                ops.saliency_backward(dm[j], amax[j], tb['pc'], tb['c2e_off'], tb['c2e_ent'], dh)
            ops.train_gates_backward(dh, dc, acts[t], cs[t], cs[t + 1], dG[t], M, hc)
            ops.cubepad_adjoint(p['dg'].dgrad(dG[t], pad4), tb['pad_off'], tb['pad_ent'], dY2[t], act=a2[t])
            ops.cubepad_adjoint(p['d2'].dgrad(dY2[t], pad4), tb['pad_off'], tb['pad_ent'], dY1[t], act=a1[t])
            if t > 0:
                ops.cubepad_adjoint(p['d1'].dgrad(dY1[t], pad1), tb['pad_off'], tb['pad_ent'], dh)   # dh_{t-1}
        self._mark('wgrad')
        f32 = dict(dtype=torch.float32, device=dev)
        g = []
        for dy, x, c_in, conv in ((dY1, xh[:T], cin + hc, cell.Conv1), (dY2, a1, 4 * hc, cell.Conv2), (dG, a2, 4 * hc, cell.Gates)):
            dw = torch.empty(tuple(conv.weight.shape), **f32)
            db = torch.empty(tuple(conv.bias.shape), **f32)
            ops.conv_wgrad(dy.view(T * n6, w, w, -1), x.reshape(T * n6, w, w, -1), c_in, tb['pad_tab'], dw, db)
            g += [dw, db]
        self._mark('wgrad_end')
        return tuple(g)


def trainer_of(cell):
    """The ClstmTraining of ``cell`` (made on first use, kept beside the module like its inference stage)."""
    tr = cell.__dict__.get('_trainer')
    if tr is None or tr.cell is not cell:
        tr = cell.__dict__['_trainer'] = ClstmTraining(cell)
    if cell.precision not in TRAIN_PRECISIONS:
        raise ValueError("training runs in precision 'fp32' or 'bf16' (got %r)" % cell.precision)
    return tr


class ClstmWindow(torch.autograd.Function):
    """maps = ClstmWindow.apply(trainer, frames, map_steps, W1, b1, W2, b2, Wg, bg): the saliency maps of ``map_steps`` of one
    training window (frames f32 [B, T, 6 w w, C], normalised).  The parameters are inputs so that autograd delivers their
    gradients to ``.grad``; the frames get none (they are data)."""

    @staticmethod
    def forward(ctx, trainer, frames, map_steps, w1, b1, w2, b2, wg, bg):
        maps, saved = trainer.forward(frames, map_steps)
        ctx.trainer, ctx.saved = trainer, saved
        return maps

    @staticmethod
    def backward(ctx, dmaps):
        grads = ctx.trainer.backward(ctx.saved, dmaps.contiguous())
        ctx.saved = None
        return (None, None, None) + grads


def window_maps(cell, frames, map_steps):
    """Differentiable saliency maps [B, len(map_steps), 2w, 4w] of one window through ``cell``."""
    tr = trainer_of(cell)
    return ClstmWindow.apply(tr, frames, tuple(map_steps), cell.Conv1.weight, cell.Conv1.bias, cell.Conv2.weight,
                             cell.Conv2.bias, cell.Gates.weight, cell.Gates.bias)
