#!/usr/bin/env python
"""Times the supervised loss (K18, csrc/suploss.hip) on one training window's worth of maps: N maps of 14 x 28 against ground truth
on the 120 x 240 loss grid, explicit fixation masks, solid-angle weights.

  forward   ops.sup_loss_forward: the resampler and K18a (one workgroup per map, three passes over the map)
  backward  ops.sup_loss_backward: the resampler, K18b (dS per grid pixel) and K18c (the adjoint, one thread per small pixel)
  both      through autograd: temporal_model.train_supervised.supervised_losses, its weighted sum, .backward()
  torch     the same through supervised_losses_torch on the GPU in float32: the definition composed from torch operations,
            forward and backward by autograd

Bytes: the least a pass must move - forward reads the maps, G and the mask once (P (4 + 1) + 4 mh mw a map); backward reads
them again and writes dmaps.  The kernels move more (S through the workspace, three passes, dS in f64): the fraction says how far
they are from one pass.

HIP events around each call, the median after warm-up, workspace reused.
  python tools/suploss_bench.py [--maps 64] [--reps 20] [--warmup 5] [--kl-eps 1e-6] [--out profiles/suploss_bench.md]
Prints a table and one JSON line; --out writes both as markdown."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def time_ms(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times), min(times)


def inputs(N, mhw, hw):
    """(maps f32 [1, N, mh, mw], gt f32 [1, N, h, w], fix u8 [1, N, h, w]) on the host: hash noise plus a blob that moves."""
    from cp_360_weakly_supervised_saliency_amd.utils import hashrng
    (mh, mw), (h, w) = mhw, hw

    def blobs(hh, ww, shift, sigma_deg):
        theta = ((2.0 * np.arange(ww) + 1.0) / ww - 1.0) * np.pi
        phi = (1.0 - (2.0 * np.arange(hh) + 1.0) / hh) * (np.pi / 2.0)
        lon = np.deg2rad(6.0 * np.arange(N) + shift)[:, None, None]
        dot = np.cos(phi)[None, :, None] * np.cos(theta[None, None, :] - lon)
        return np.exp((dot - 1.0) / np.deg2rad(sigma_deg) ** 2)

    gt = blobs(h, w, 0.0, 10.0) + 0.05 * hashrng.uniform(71, (N, h, w), dtype=np.float64)
    maps = blobs(mh, mw, 15.0, 18.0) + 0.2 * hashrng.uniform(72, (N, mh, mw), dtype=np.float64)
    fix = (gt >= np.quantile(gt.reshape(N, -1), 0.97, axis=1)[:, None, None]).astype(np.uint8)
    return maps.astype(np.float32)[None], gt.astype(np.float32)[None], fix[None]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--maps', type=int, default=64)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--kl-eps', type=float, default=1e-6)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from cp_360_weakly_supervised_saliency_amd import ops
    from cp_360_weakly_supervised_saliency_amd.temporal_model import train_supervised as ts

    assert torch.cuda.is_available(), "suploss_bench needs a GPU"
    N, mhw, hw, eps = args.maps, (14, 28), (120, 240), args.kl_eps
    P, p = hw[0] * hw[1], mhw[0] * mhw[1]
    maps, gt, fix = (torch.from_numpy(v).cuda() for v in inputs(N, mhw, hw))
    m, g, fx = maps[0], gt[0], fix[0]
    a = ops.sphere_eval_weights(hw[0], 'solid_angle', m.device)
    work = ops.sup_loss_work(N, mhw, hw, m.device)
    terms, valid, stats = ops.sup_loss_forward(m, g, a, fx, eps, work=work)
    gterms = torch.tensor([1.0 / N, -1.0 / N, -0.1 / N], dtype=torch.float64, device=m.device).repeat(N, 1)
    weigh = lambda kl, cc, nss: kl - cc - 0.1 * nss

    def both(losses, x):
        x.grad = None
        kl, cc, nss, _ = losses(x, gt, fix, kl_eps=eps)
        weigh(kl, cc, nss).backward()
        return kl, cc, nss, x.grad

    x_dev, x_torch = maps.clone().requires_grad_(True), maps.clone().requires_grad_(True)
    got, want = both(ts.supervised_losses, x_dev), both(ts.supervised_losses_torch, x_torch)
    term_gap = max(abs(float(u) - float(v)) / max(1.0, abs(float(v))) for u, v in zip(got[:3], want[:3]))
    grad_gap = float((got[3] - want[3]).abs().max() / want[3].abs().max())

    ms_f, min_f = time_ms(lambda: ops.sup_loss_forward(m, g, a, fx, eps, work=work), args.reps, args.warmup)
    ms_b, min_b = time_ms(lambda: ops.sup_loss_backward(m, g, a, stats, valid, gterms, fx, eps, work=work), args.reps, args.warmup)
    ms_d, min_d = time_ms(lambda: both(ts.supervised_losses, x_dev), args.reps, args.warmup)
    ms_t, min_t = time_ms(lambda: both(ts.supervised_losses_torch, x_torch), args.reps, args.warmup)
    ghz = ops.held_clock_ghz()
    bytes_f, bytes_b = N * (5.0 * P + 4.0 * p), N * (5.0 * P + 8.0 * p)
    res = {'tool': 'suploss_bench', 'maps': N, 'map_hw': list(mhw), 'grid': list(hw), 'kl_eps': eps, 'reps': args.reps,
           'warmup': args.warmup, 'valid_maps': [int(v) for v in valid.sum(dim=0).tolist()],
           'forward_ms': ms_f, 'forward_min_ms': min_f, 'backward_ms': ms_b, 'backward_min_ms': min_b,
           'kernels_ms': ms_f + ms_b, 'autograd_ms': ms_d, 'autograd_min_ms': min_d, 'torch_ms': ms_t, 'torch_min_ms': min_t,
           'torch_over_kernels': ms_t / (ms_f + ms_b), 'torch_over_autograd': ms_t / ms_d,
           'forward_least_bytes': bytes_f, 'backward_least_bytes': bytes_b, 'forward_GBps_of_least': bytes_f / (ms_f * 1e-3) / 1e9,
           'backward_GBps_of_least': bytes_b / (ms_b * 1e-3) / 1e9, 'terms_apart_from_torch': term_gap,
           'gradient_apart_from_torch': grad_gap, 'held_clock_ghz': ghz, 'work_KB': work.numel() * 8 / 1e3}
    lines = ['N = %d maps of %d x %d against %d x %d, explicit masks, solid-angle weights, kl_eps = %g; %s maps valid (kl, cc, nss)'
             % (N, mhw[0], mhw[1], hw[0], hw[1], eps, res['valid_maps']),
             'median of %d after %d warm-up calls (HIP events); held clock %.2f GHz' % (args.reps, args.warmup, ghz),
             'forward  (resample, K18a)        %9.3f ms / call (min %.3f)   %.1f GB/s of the least bytes' % (ms_f, min_f, res['forward_GBps_of_least']),
             'backward (resample, K18b, K18c)  %9.3f ms / call (min %.3f)   %.1f GB/s of the least bytes' % (ms_b, min_b, res['backward_GBps_of_least']),
             'forward + backward, kernels      %9.3f ms' % (ms_f + ms_b),
             'supervised_losses + .backward()  %9.3f ms / call (min %.3f)   the same through autograd' % (ms_d, min_d),
             'supervised_losses_torch (f32)    %9.3f ms / call (min %.3f)   %.1f x the kernels, %.1f x the autograd call'
             % (ms_t, min_t, res['torch_over_kernels'], res['torch_over_autograd']),
             'torch float32 against the kernels: terms apart %.2e (relative), gradient apart %.2e of its largest' % (term_gap, grad_gap),
             'workspace                        %9.1f KB' % res['work_KB']]
    print('\n'.join(lines))
    print(json.dumps(res))
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write('# tools/suploss_bench.py on one MI355X\n\n```\n' + '\n'.join(lines) + '\n```\n\nThe JSON line of the run:\n\n```\n'
                     + json.dumps(res) + '\n```\n')


if __name__ == '__main__':
    main()
