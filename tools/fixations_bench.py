#!/usr/bin/env python
"""Times the fixation kernels (K15, csrc/fixations.hip) on one video per call: F frames of 120 x 240, 32 viewers per frame,
sigma 5 degrees.

  counts    ops.fixation_counts: a clear and one launch
  density   ops.fixation_density: the tables and one launch; F P viewers (pixel, point) pairs, one expf each, set against the
            rate at which the chip issues v_exp_f32: one wave-instruction per 8 clocks and SIMD = 8 lanes x 4 SIMDs x CUs x the
            held clock (1.0 would be a loop of nothing but the exponential's one hardware instruction; expf itself is that
            instruction plus its range reduction, and a pair adds the dot product)
  sAUC      FixationMaps.shuffled_auc with 'other_frames' negatives on maps already on the grid: the negatives made with torch,
            one resampling copy and the three launches of cp360_fix_sauc - and ops.shuffled_auc alone

HIP events around each call, the median after warm-up, workspace reused.
  python tools/fixations_bench.py [--frames 256] [--viewers 32] [--reps 20] [--warmup 5] [--out profiles/fixations_bench.md]
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


def points(F, viewers):
    """Per frame a target (longitude uniform, latitude normal with 12 degrees) and `viewers` points normal around it with 6 degrees."""
    from cp_360_weakly_supervised_saliency_amd.utils import hashrng
    t_lon = hashrng.uniform(41, (F,), -np.pi, np.pi, dtype=np.float64)
    t_lat = np.deg2rad(12.0) * hashrng.normal(42, (F,), dtype=np.float64)
    d = np.deg2rad(6.0) * hashrng.normal(43, (F, viewers, 2), dtype=np.float64)
    lonlat = np.stack([t_lon[:, None] + d[:, :, 0] / np.cos(t_lat)[:, None], t_lat[:, None] + d[:, :, 1]], -1).reshape(-1, 2)
    return np.ascontiguousarray(lonlat), (np.arange(F + 1) * viewers).astype(np.int32)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--frames', type=int, default=256)
    ap.add_argument('--viewers', type=int, default=32)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from cp_360_weakly_supervised_saliency_amd import ops
    from cp_360_weakly_supervised_saliency_amd.utils import fixations

    assert torch.cuda.is_available(), "fixations_bench needs a GPU"
    F, V, h, w, sigma_deg = args.frames, args.viewers, 120, 240, 5.0
    P = h * w
    lonlat_np, offsets_np = points(F, V)
    lonlat, offsets = torch.from_numpy(lonlat_np).cuda(), torch.from_numpy(offsets_np).cuda()
    fm = fixations.FixationMaps((h, w), sigma_deg)
    counts, n_points = fm.counts(lonlat, offsets)
    sal = fm.density(lonlat, offsets)
    auc, c_tot, a_neg = fm.shuffled_auc(sal, counts)
    assert n_points.tolist() == [V] * F and not bool(torch.isnan(auc).any())
    n_pos = (counts > 0).sum(dim=(1, 2)).cpu().numpy()
    res = {'tool': 'fixations_bench', 'frames': F, 'viewers': V, 'grid': [h, w], 'sigma_deg': sigma_deg, 'reps': args.reps,
           'warmup': args.warmup, 'mean_sauc_of_the_density': float(auc.mean()),
           'fixated_pixels': {'min': int(n_pos.min()), 'mean': float(n_pos.mean()), 'max': int(n_pos.max())}}
    sigma = float(np.deg2rad(sigma_deg))
    work = ops.fixation_work(F, h, w, lonlat.device)
    neg = (counts.sum(dim=0, keepdim=True) - counts).to(torch.int32).contiguous()
    ms_c, _ = time_ms(lambda: ops.fixation_counts(lonlat, offsets, (h, w)), args.reps, args.warmup)
    ms_d, min_d = time_ms(lambda: ops.fixation_density(lonlat, offsets, (h, w), sigma, work=work), args.reps, args.warmup)
    ms_s, _ = time_ms(lambda: fm.shuffled_auc(sal, counts), args.reps, args.warmup)
    ms_k, _ = time_ms(lambda: ops.shuffled_auc(sal, counts, neg, work=work), args.reps, args.warmup)
    ghz = ops.held_clock_ghz()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    pairs = float(F) * P * V
    exp_rate = 8.0 * 4.0 * cus * ghz * 1e9
    res.update({'counts_ms': ms_c, 'density_ms': ms_d, 'density_min_ms': min_d, 'sauc_ms': ms_s, 'sauc_kernels_ms': ms_k,
                'pairs': pairs, 'pairs_per_s': pairs / (ms_d * 1e-3), 'held_clock_ghz': ghz, 'cus': cus,
                'v_exp_issue_per_s': exp_rate, 'pairs_over_v_exp_issue': pairs / (ms_d * 1e-3) / exp_rate,
                'work_MB': work.numel() * 8 / 1e6})
    lines = ['F = %d frames of %d x %d, %d viewers per frame, sigma %g degrees; fixated pixels per frame %d .. %d, mean %.1f'
             % (F, h, w, V, sigma_deg, n_pos.min(), n_pos.max(), n_pos.mean()),
             'median of %d after %d warm-up calls (HIP events); held clock %.2f GHz, %d CUs' % (args.reps, args.warmup, ghz, cus),
             'counts                               %8.3f ms / call' % ms_c,
             'density                              %8.3f ms / call   %.3e pairs, %.3e pairs / s = %.3f of %.3e v_exp_f32 lanes / s'
             % (ms_d, pairs, res['pairs_per_s'], res['pairs_over_v_exp_issue'], exp_rate),
             "sAUC, 'other_frames' negatives       %8.3f ms / call   (negatives with torch, a resampling copy, 3 launches)" % ms_s,
             '  cp360_fix_sauc alone               %8.3f ms / call' % ms_k,
             '  workspace                          %8.1f MB' % res['work_MB']]
    print('\n'.join(lines))
    print(json.dumps(res))
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write('# tools/fixations_bench.py on one MI355X\n\n```\n' + '\n'.join(lines) + '\n```\n\nThe JSON line of the run:\n\n```\n'
                     + json.dumps(res) + '\n```\n')


if __name__ == '__main__':
    main()
