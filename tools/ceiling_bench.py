#!/usr/bin/env python
"""Times the point scores behind the human ceiling and the prior baselines (K19, csrc/fixations.hip) on one video: F frames of
120 x 240, V viewers per frame, sigma 5 degrees.

  ceiling   FixationMaps.ceiling: leave-one-out, per chunk of 256 frames the tables, the f64 totals (K19a) and the scores (K19b),
            then the torch means; F V P (point, pixel) pairs, two expf each in K19b and one in K19a
  score     FixationMaps.score_points on maps already on the grid and on the device: per chunk a resampling copy and K19b
  torch     the same definition composed with torch on the first --slice frames, a frame at a time ([n, P] terms, their f64 sum,
            the n leave-one-out maps, the weighted moments and the comparisons): set beside `ceiling` by rate, pairs per second

HIP events around each call, the median after warm-up, workspace reused.  --step runs one of the three, so that each can run
under a time limit of its own:
  for s in ceiling score torch; do timeout -k 10 600 python tools/ceiling_bench.py --step $s --out profiles/fixations_bench.md; done
Prints a table and one JSON line; --out appends both as markdown."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.fixations_bench import points, time_ms                     # noqa: E402  the same viewers, the same timer


def torch_ceiling(lonlat, offsets, hw, sigma_deg, a_rows):
    """The definition with torch, a frame at a time -> f64 [N, 2]; finite points only."""
    import torch
    h, w = hw
    dev = lonlat.device
    theta = ((2.0 * torch.arange(w, device=dev, dtype=torch.float64) + 1.0) / w - 1.0) * np.pi
    phi = (1.0 - (2.0 * torch.arange(h, device=dev, dtype=torch.float64) + 1.0) / h) * (np.pi / 2.0)
    p = torch.stack([(phi.cos()[:, None] * theta.cos()[None]), phi.sin()[:, None].expand(h, w), (phi.cos()[:, None] * theta.sin()[None])],
                    -1).reshape(-1, 3).float()
    a = a_rows.to(torch.float64).repeat_interleave(w)
    A = a.sum()
    kappa = float(np.float32(1.0 / np.deg2rad(sigma_deg) ** 2))
    out = []
    for f in range(len(offsets) - 1):
        q = lonlat[offsets[f]:offsets[f + 1]]
        lon, lat = q[:, 0], q[:, 1]
        x = torch.floor((lon / np.pi + 1.0) * (w / 2.0)).remainder(w).long()
        y = torch.floor((1.0 - lat / (np.pi / 2.0)) * (h / 2.0)).clamp(0, h - 1).long()
        i = y * w + x
        d = torch.stack([lat.cos() * lon.cos(), lat.sin(), lat.cos() * lon.sin()], -1).float()
        e = torch.exp(kappa * (d @ p.T - 1.0)).double()                # [n, P]
        l = (e.sum(dim=0, keepdim=True) - e).clamp(min=0.0)
        li = l.gather(1, i[:, None])
        mu = (l * a).sum(dim=1, keepdim=True) / A
        sigma = (((l - mu) ** 2 * a).sum(dim=1, keepdim=True) / A).sqrt()
        a_i = a[i][:, None]
        a_k = ((l >= li) * a).sum(dim=1, keepdim=True) - a_i           # the point's own pixel compares equal: taken out
        a_neg = A - a_i
        out.append(torch.cat([(2.0 * a_neg - a_k) / (2.0 * a_neg), (li - mu) / sigma], dim=1))
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--frames', type=int, default=1800)
    ap.add_argument('--viewers', type=int, default=48)
    ap.add_argument('--slice', type=int, default=30)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--step', choices=['ceiling', 'score', 'torch', 'all'], default='all')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from cp_360_weakly_supervised_saliency_amd import ops
    from cp_360_weakly_supervised_saliency_amd.utils import fixations

    assert torch.cuda.is_available(), "ceiling_bench needs a GPU"
    F, V, h, w, sigma_deg = args.frames, args.viewers, 120, 240, 5.0
    P = h * w
    lonlat_np, offsets_np = points(F, V)
    lonlat = torch.from_numpy(lonlat_np).cuda()
    fm = fixations.FixationMaps((h, w), sigma_deg)
    ghz = ops.held_clock_ghz()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    pairs = float(F) * V * P
    res = {'tool': 'ceiling_bench', 'step': args.step, 'frames': F, 'viewers': V, 'grid': [h, w], 'sigma_deg': sigma_deg,
           'reps': args.reps, 'warmup': args.warmup, 'pairs': pairs, 'held_clock_ghz': ghz, 'cus': cus}
    lines = ['F = %d frames of %d x %d, %d viewers per frame, sigma %g degrees: %.3e (point, pixel) pairs' % (F, h, w, V, sigma_deg, pairs),
             'median of %d after %d warm-up calls (HIP events); held clock %.2f GHz, %d CUs' % (args.reps, args.warmup, ghz, cus)]
    if args.step in ('ceiling', 'all'):
        top = fm.ceiling(lonlat, offsets_np)
        ms, mn = time_ms(lambda: fm.ceiling(lonlat, offsets_np), args.reps, args.warmup)
        res.update({'ceiling_ms': ms, 'ceiling_min_ms': mn, 'ceiling_pairs_per_s': pairs / (ms * 1e-3), 'work_MB': fm._work.numel() * 8 / 1e6,
                    'ceiling_auc': float(top.video_auc), 'ceiling_nss': float(top.video_nss)})
        lines += ['.ceiling                             %8.3f ms / call   %.3e pairs / s   (AUC %.4f, NSS %.2f; workspace %.1f MB)'
                  % (ms, res['ceiling_pairs_per_s'], res['ceiling_auc'], res['ceiling_nss'], res['work_MB'])]
    if args.step in ('score', 'all'):
        sal = fm.density(lonlat, offsets_np, None)
        mine = fm.score_points(sal, lonlat, offsets_np)
        ms, mn = time_ms(lambda: fm.score_points(sal, lonlat, offsets_np), args.reps, args.warmup)
        res.update({'score_ms': ms, 'score_min_ms': mn, 'score_pairs_per_s': pairs / (ms * 1e-3), 'own_auc': float(mine.video_auc),
                    'own_nss': float(mine.video_nss)})
        lines += ['.score_points, the own densities     %8.3f ms / call   %.3e pairs / s   (AUC %.4f, NSS %.2f)'
                  % (ms, res['score_pairs_per_s'], res['own_auc'], res['own_nss'])]
    if args.step in ('torch', 'all'):
        Fs = min(args.slice, F)
        sl, so = lonlat[:Fs * V], offsets_np[:Fs + 1]
        a = ops.sphere_eval_weights(h, 'solid_angle', lonlat.device)
        got = fm.ceiling(sl, so)
        ref = torch_ceiling(sl, so, (h, w), sigma_deg, a)
        apart = float((torch.stack([got.auc, got.nss], 1) - ref).abs().max())
        ms_t, _ = time_ms(lambda: torch_ceiling(sl, so, (h, w), sigma_deg, a), args.reps, args.warmup)
        ms_k, _ = time_ms(lambda: fm.ceiling(sl, so), args.reps, args.warmup)
        sp = float(Fs) * V * P
        res.update({'slice_frames': Fs, 'torch_ms': ms_t, 'torch_pairs_per_s': sp / (ms_t * 1e-3), 'slice_ceiling_ms': ms_k,
                    'slice_ceiling_pairs_per_s': sp / (ms_k * 1e-3), 'slice_apart': apart})
        lines += ['torch, %3d frames                    %8.3f ms / call   %.3e pairs / s' % (Fs, ms_t, res['torch_pairs_per_s']),
                  '.ceiling, the same frames            %8.3f ms / call   %.3e pairs / s   (the two apart %.1e at most)'
                  % (ms_k, res['slice_ceiling_pairs_per_s'], apart)]
    print('\n'.join(lines))
    print(json.dumps(res))
    if args.out:
        with open(args.out, 'a') as fh:
            fh.write('\n# tools/ceiling_bench.py --step %s on one MI355X\n\n```\n' % args.step + '\n'.join(lines)
                     + '\n```\n\nThe JSON line of the run:\n\n```\n' + json.dumps(res) + '\n```\n')


if __name__ == '__main__':
    main()
