#!/usr/bin/env python3
"""ConvLSTM training throughput (temporal_model/train_temporal.py): one JSON line with ms per iteration and iterations/s of
train_step at Hc = 1000, w = 7, seq_len 5 (maps of steps 1..4), fp32 and bf16, B = 1 and 4, and the phase split of an
iteration timed with HIP events: forward, flow resize, loss forward, loss backward, BPTT (dgrad), wgrad, Adam, weight repack
("loss_total" spans the loss forward, the loss backward and the autograd work between them).  The flow is given on the host
at --flow H x W (default 28 x 56, the loss resolution of the default --flow-h 28: the rows of earlier measurements) and
resized to flow_h x 2 flow_h on the device.  "torch_loss_ms" is the torch ``flow_losses`` forward + backward on the same maps
and flows, timed standalone ("hip_loss_ms": the HIP loss the same way); "loss_bound_us" is the loss's paper bound (the flow it
reads at the HBM rate, once per direction).  Flops and bytes of the other phases are computed from the shapes below.  Kernel
times: run this under `rocprofv3 --kernel-trace --stats` (a separate run: --configs bf16:4 --steps 1 --warmup 1).

    python tools/train_bench.py [--steps 5] [--warmup 2] [--configs fp32:1,fp32:4,bf16:1,bf16:4] [--flow 480x960 --flow-h 480]
                                [--optimizer torch|fused]
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cp_360_weakly_supervised_saliency_amd.model.clstm import ConvLSTMCell  # noqa: E402
from cp_360_weakly_supervised_saliency_amd.model.clstm_train import trainer_of  # noqa: E402
from cp_360_weakly_supervised_saliency_amd.temporal_model import train_temporal as tt  # noqa: E402
from cp_360_weakly_supervised_saliency_amd.utils import hashrng, synth  # noqa: E402

HC, W, T, L = 1000, 7, 5, 3
PEAK = {'fp32': 157.3e12, 'bf16': 2.5e15}          # dense MFMA, MI355X spec
HBM = 6.3e12                                       # measured copy bandwidth


def work(B, precision):
    """Flops / main bytes per iteration from the shapes (Conv1 2Hc -> 4Hc, Conv2 and Gates 4Hc -> 4Hc, 3x3, 7x7 faces)."""
    M, Mpad = 6 * B * W * W, 6 * B * (W + 2) ** 2
    es = 4 if precision == 'fp32' else 2
    k1, k2 = 9 * 2 * HC, 9 * 4 * HC
    fwd = T * 2.0 * M * 4 * HC * (k1 + 2 * k2)
    dgrad = T * 2.0 * Mpad * 9 * 4 * HC * (4 * HC + 4 * HC + HC)     # full correlation onto the padded grid: Gates, Conv2, Conv1's hidden half
    wgrad = 2.0 * T * M * 4 * HC * (k1 + 2 * k2)
    n_w = 4 * HC * (k1 + 2 * k2)
    return dict(forward_flop=fwd, dgrad_flop=dgrad, wgrad_flop=wgrad,
                forward_bytes=T * n_w * es, dgrad_bytes=T * 9 * 4 * HC * (9 * HC) * es, wgrad_bytes=4.0 * n_w,
                adam_bytes=4.0 * n_w * 7, repack_bytes=n_w * (4 + es) * 2)


def loss_bytes(B, flow_h):
    """Paper bytes of the flow loss: the scaled flow read once per direction, the backward's row sums written and read."""
    pairs, h, wl = B * L, flow_h, 2 * flow_h
    return dict(fwd=pairs * h * wl * 8.0, bwd=pairs * h * wl * 8.0 + 2 * pairs * h * 4 * W * 4.0)


def time_loss(fn, maps, steps, warmup):
    """Median ms of fn(maps) forward + backward, HIP events, standalone."""
    ts = []
    for it in range(warmup + steps):
        m = maps.detach().clone().requires_grad_(True)
        s = torch.cuda.Event(enable_timing=True)
        e = torch.cuda.Event(enable_timing=True)
        s.record()
        terms = fn(m)
        (0.7 * terms[0] + terms[1] + 0.01 * terms[2]).backward()
        e.record()
        torch.cuda.synchronize()
        if it >= warmup:
            ts.append(s.elapsed_time(e))
    return float(np.median(ts))


def run(precision, B, steps, warmup, flow_hw, flow_h, optimizer='torch'):
    cell = ConvLSTMCell(HC, HC, precision=precision)
    cell.load_state_dict({k: torch.from_numpy(v) for k, v in synth.clstm_state(seed=2, input_size=HC, hidden_size=HC).items()})
    cell.cuda()
    opt = (tt.FusedAdam(cell, lr=1e-6) if optimizer == 'fused' else torch.optim.Adam(cell.parameters(), lr=1e-6))
    cfg = types.SimpleNamespace(seq_len=T, flow_h=flow_h, l_s=0.7, l_t=1.0, l_m=0.01, mm_th=0.15)
    seq = torch.from_numpy(np.stack([synth.cam_clip(9000 + b, T) for b in range(B)])).cuda()       # [B, T, 6, C, 7, 7]
    # on the host, as a data loader gives it; 0.25 px (std) once scaled by flow_h / W, as the 28 x 56 rows had
    flow = torch.from_numpy(hashrng.normal(9100, (B, T) + flow_hw + (2,), 0, 0.25 * flow_hw[1] / flow_h))
    tr = trainer_of(cell)
    phases = {k: [] for k in ('forward', 'resize', 'loss', 'loss_bwd', 'loss_total', 'bptt', 'wgrad', 'adam', 'repack')}
    total = []
    for it in range(warmup + steps):
        tr.events = ev = []
        e0 = torch.cuda.Event(enable_timing=True)
        e0.record()
        step = opt.step

        def timed_step(*a, **k):
            s = torch.cuda.Event(enable_timing=True)
            s.record()
            r = step(*a, **k)
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            ev.extend([('adam', s), ('adam_end', e)])
            return r
        opt.step = timed_step
        tt.train_step(cell, seq, flow, opt, cfg)
        opt.step = step
        s = torch.cuda.Event(enable_timing=True)
        s.record()
        tr.plans()                                     # the repack the next iteration would do first
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        torch.cuda.synchronize()
        tr.events = None
        if it < warmup:
            continue
        d = dict(ev)
        total.append(e0.elapsed_time(e1))
        phases['forward'].append(d['forward'].elapsed_time(d['forward_end']))
        phases['resize'].append(d['resize'].elapsed_time(d['resize_end']))
        phases['loss'].append(d['loss'].elapsed_time(d['loss_end']))
        phases['loss_bwd'].append(d['loss_bwd'].elapsed_time(d['loss_bwd_end']))
        phases['loss_total'].append(d['forward_end'].elapsed_time(d['bptt']))
        phases['bptt'].append(d['bptt'].elapsed_time(d['wgrad']))
        phases['wgrad'].append(d['wgrad'].elapsed_time(d['wgrad_end']))
        phases['adam'].append(d['adam'].elapsed_time(d['adam_end']))
        phases['repack'].append(s.elapsed_time(e1))
    med = lambda a: float(np.median(a))
    ms = med(total)
    wk = work(B, precision)
    out = dict(precision=precision, B=B, optimizer=optimizer, ms_per_iter=round(ms, 2), iters_per_s=round(1000.0 / ms, 3),
               phases_ms={k: round(med(v), 2) for k, v in phases.items()})
    for ph in ('forward', 'bptt', 'wgrad'):
        key = 'dgrad' if ph == 'bptt' else ph
        t = med(phases[ph]) * 1e-3
        f, b = wk[key + '_flop'], wk[key + '_bytes']
        out[ph + '_tflops'] = round(f / t / 1e12, 2)
        out[ph + '_tbps'] = round(b / t / 1e12, 2)
        out[ph + '_bound_fraction'] = round(max(f / PEAK[precision], b / HBM) / t, 3)
    # the fused step also writes every pack the plan holds: the forward layouts that exist and the three dgrad operands
    plan = tr.plans()
    pack_bytes = sum(t.numel() * t.element_size() for c in ('c1', 'c2', 'g') for t in plan[c]._packed.values()) + \
        sum(plan[k].packed.numel() * plan[k].packed.element_size() for k in ('d1', 'd2', 'dg'))
    out['pack_bytes'] = int(pack_bytes)
    adam_bytes = wk['adam_bytes'] + (pack_bytes if optimizer == 'fused' else 0)
    out['adam_bytes'] = int(adam_bytes)
    out['adam_tbps'] = round(adam_bytes / (med(phases['adam']) * 1e-3) / 1e12, 2)
    out['adam_share'] = round(med(phases['adam']) / ms, 3)
    # the loss alone, before (torch flow_losses) and after (HIP), on the same maps and resized flows
    with torch.no_grad():
        maps = torch.rand((B, L + 1, 2 * W, 4 * W), generator=torch.Generator().manual_seed(5)).cuda()
    scaled = tt.resize_flow(flow[:, 1:1 + L].cuda().contiguous(), flow_h)
    sub = types.SimpleNamespace(flow_h=flow_h, mm_th=cfg.mm_th, seq_len=L + 1)
    out['torch_loss_ms'] = round(time_loss(lambda m: tt.flow_losses(m, 2.0 * scaled, sub, L), maps, steps, warmup), 3)
    out['hip_loss_ms'] = round(time_loss(lambda m: tt.device_flow_losses(m, scaled, cfg, L), maps, steps, warmup), 3)
    out['loss_bound_us'] = {k: round(v / HBM * 1e6, 2) for k, v in loss_bytes(B, flow_h).items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--configs', default='fp32:1,fp32:4,bf16:1,bf16:4')
    ap.add_argument('--flow', default='28x56', help='flow H x W as stored (the loader\'s resolution)')
    ap.add_argument('--flow-h', type=int, default=28, help='cfg.flow_h: the loss resolution is flow_h x 2 flow_h')
    ap.add_argument('--optimizer', choices=('torch', 'fused'), default='torch',
                    help='torch.optim.Adam, or train_temporal.FusedAdam (the step also writes the packs: no repack)')
    a = ap.parse_args()
    flow_hw = tuple(int(v) for v in a.flow.lower().split('x'))
    t0 = time.time()
    res = [run(p, int(b), a.steps, a.warmup, flow_hw, a.flow_h, a.optimizer) for p, b in (c.split(':') for c in a.configs.split(','))]
    print(json.dumps(dict(metric='clstm_train', hidden=HC, face=W, seq_len=T, flow=list(flow_hw), flow_h=a.flow_h,
                          steps=a.steps, warmup=a.warmup, optimizer=a.optimizer,
                          device=torch.cuda.get_device_name(0), wall_s=round(time.time() - t0, 1), results=res)))


if __name__ == '__main__':
    main()
