#!/usr/bin/env python
"""Times the sphere-weighted metrics (K14, csrc/sphere_eval.hip) on a video per call next to K8's per-frame functions, on the
same maps: F predictions of 14 x 28 and F ground-truth maps of 120 x 240 on the 120 x 240 grid.

  SphereEval.evaluate   two resamplings and the three launches of cp360_seval_scores, device tensors in, nothing copied back;
                        HIP events around each call, the median after warm-up, workspace reused
  scores alone          ops.sphere_eval on maps already on the grid - and once more with an empty fixation mask, where every
                        workgroup of the rank kernel (K14b) exits at once: the difference is the rank kernel's time, and
                        sum_f n_fix_f P pair compares over it the rate set against 64 lanes x 4 SIMDs x CUs x the held clock
                        (one compare-select-add per lane and clock would be 1.0; a pair costs two, >= and >)
  K8 per frame          eval_saliency.AUC_Judd(jitter=False) + CorrCoeff + similarity, frame by frame, on the same device
                        tensors and on numpy maps (the reference's way); a host clock around the calls, which end in .item() /
                        .cpu() and so wait for the device

  python tools/eval_bench.py [--frames 256] [--k8-frames 32] [--reps 20] [--warmup 5] [--out profiles/eval_bench.md]
Prints a table and one JSON line; --out writes both as markdown."""
import argparse
import json
import os
import statistics
import sys
import time

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


def maps(F, hs, ws, hg, wg):
    """(sal f32 [F, hs, ws], gt f32 [F, hg, wg]): three blobs of 12 degrees on hash noise per ground-truth frame, the prediction
    two wider blobs nearby - vectorised over the frames, the kind of input tests/sphere_eval_restate.video makes."""
    from cp_360_weakly_supervised_saliency_amd.utils import hashrng

    def dirs(h, w):
        theta = ((2.0 * np.arange(w) + 1.0) / w - 1.0) * np.pi
        phi = (1.0 - (2.0 * np.arange(h) + 1.0) / h) * (np.pi / 2.0)
        return np.stack([np.cos(phi)[:, None] * np.cos(theta)[None, :], np.sin(phi)[:, None] * np.ones(w)[None, :],
                         np.cos(phi)[:, None] * np.sin(theta)[None, :]], axis=-1)

    cen = hashrng.normal(31, (F, 3, 3), dtype=np.float64)
    cen /= np.linalg.norm(cen, axis=2, keepdims=True)
    near = cen + 0.18 * hashrng.normal(32, (F, 3, 3), dtype=np.float64)
    near /= np.linalg.norm(near, axis=2, keepdims=True)
    gt = 0.05 * hashrng.uniform(33, (F, hg, wg), dtype=np.float64)
    sal = 0.2 * hashrng.uniform(34, (F, hs, ws), dtype=np.float64)
    kg, ks = 1.0 / np.deg2rad(12.0) ** 2, 1.0 / np.deg2rad(18.0) ** 2
    gt += np.exp(kg * (np.einsum('hwc,fkc->fkhw', dirs(hg, wg), cen) - 1.0)).sum(axis=1)
    sal += np.exp(ks * (np.einsum('hwc,fkc->fkhw', dirs(hs, ws), near[:, :2]) - 1.0)).sum(axis=1)
    return sal.astype(np.float32), gt.astype(np.float32)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--frames', type=int, default=256)
    ap.add_argument('--k8-frames', type=int, default=32)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from cp_360_weakly_supervised_saliency_amd import ops
    from cp_360_weakly_supervised_saliency_amd.utils import eval_saliency, eval_sphere

    assert torch.cuda.is_available(), "eval_bench needs a GPU"
    F, h, w = args.frames, 120, 240
    P = h * w
    sal_np, gt_np = maps(F, 14, 28, h, w)
    sal, gt = torch.from_numpy(sal_np).cuda(), torch.from_numpy(gt_np).cuda()
    ev = eval_sphere.SphereEval((h, w))
    r = ev.evaluate(sal, gt)
    n_fix = r.n_fix.cpu().numpy().astype(np.int64)
    assert bool(torch.isfinite(r.scores).all()) and n_fix.min() > 0 and n_fix.max() < P
    means = ev.means(r)
    res = {'tool': 'eval_bench', 'frames': F, 'grid': [h, w], 'reps': args.reps, 'warmup': args.warmup,
           'n_fix': {'min': int(n_fix.min()), 'mean': float(n_fix.mean()), 'max': int(n_fix.max())}, 'means': means}
    # K14, the driver and its parts
    ms, fastest = time_ms(lambda: ev.evaluate(sal, gt), args.reps, args.warmup)
    res['evaluate'] = {'ms_per_call': ms, 'min_ms': fastest, 'frames_per_s': F / (ms * 1e-3), 'us_per_frame': 1e3 * ms / F}
    S, G = ev.resample(sal), ev.resample(gt)
    work = ops.sphere_eval_work(F, h, w, S.device)
    none = torch.zeros((F, h, w), dtype=torch.uint8, device=S.device)
    ms_res, _ = time_ms(lambda: (ev.resample(sal), ev.resample(gt)), args.reps, args.warmup)
    ms_sc, _ = time_ms(lambda: ops.sphere_eval(S, G, ev.weights, work=work), args.reps, args.warmup)
    ms_no, _ = time_ms(lambda: ops.sphere_eval(S, G, ev.weights, fixations=none, work=work), args.reps, args.warmup)
    ghz = ops.held_clock_ghz()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    pairs = float(n_fix.sum()) * P
    ms_rank = max(ms_sc - ms_no, 1e-6)
    lane_rate = 64.0 * 4.0 * cus * ghz * 1e9
    res['parts'] = {'resample_ms': ms_res, 'scores_ms': ms_sc, 'scores_without_fixations_ms': ms_no, 'rank_ms': ms_rank,
                    'pairs': pairs, 'pairs_per_s': pairs / (ms_rank * 1e-3), 'held_clock_ghz': ghz, 'cus': cus,
                    'lane_ops_per_s': lane_rate, 'pairs_over_lane_ops': pairs / (ms_rank * 1e-3) / lane_rate,
                    'work_MB': work.numel() * 8 / 1e6, 'launches': 3}
    # K8, frame by frame
    n8 = min(args.k8_frames, F)

    def k8(maps_s, maps_g):
        out = []
        for f in range(n8):
            out.append((eval_saliency.AUC_Judd(maps_s[f], maps_g[f], jitter=False), eval_saliency.CorrCoeff(maps_s[f], maps_g[f]),
                        eval_saliency.similarity(maps_s[f], maps_g[f])))
        return out

    res['k8'] = {}
    for name, (ms_, mg_) in (('device tensors', (sal, gt)), ('numpy maps', (sal_np, gt_np))):
        k8(ms_, mg_)                                                   # warm-up
        torch.cuda.synchronize()
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            k8(ms_, mg_)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        t = statistics.median(times)
        res['k8'][name] = {'frames': n8, 'ms_per_frame': 1e3 * t / n8, 'frames_per_s': n8 / t,
                           'evaluate_speedup': (t / n8) / (ms * 1e-3 / F)}
    e, p = res['evaluate'], res['parts']
    lines = ['F = %d, predictions 14 x 28, ground truth 120 x 240, grid 120 x 240, solid-angle weights; n_fix %d .. %d, mean %.0f'
             % (F, res['n_fix']['min'], res['n_fix']['max'], res['n_fix']['mean']),
             'median of %d after %d warm-up calls (HIP events); held clock %.2f GHz, %d CUs' % (args.reps, args.warmup, ghz, cus),
             'SphereEval.evaluate              %8.3f ms / call   %8.2f us / frame   %10.0f frames / s' % (e['ms_per_call'], e['us_per_frame'], e['frames_per_s']),
             '  two resamplings                %8.3f ms' % p['resample_ms'],
             '  scores (3 launches)            %8.3f ms' % p['scores_ms'],
             '  scores, empty fixation masks   %8.3f ms   (K14a and K14c; every K14b workgroup exits)' % p['scores_without_fixations_ms'],
             '  K14b by difference             %8.3f ms   %.3e pairs, %.3e pairs / s = %.3f of %.3e lane-ops / s'
             % (p['rank_ms'], p['pairs'], p['pairs_per_s'], p['pairs_over_lane_ops'], p['lane_ops_per_s']),
             '  workspace                      %8.1f MB' % p['work_MB']]
    for name, d in res['k8'].items():
        lines.append('K8 AUC_Judd(jitter=False) + CorrCoeff + similarity, %-15s %8.3f ms / frame %8.0f frames / s   evaluate is %.0f x'
                     % (name + ':', d['ms_per_frame'], d['frames_per_s'], d['evaluate_speedup']))
    print('\n'.join(lines))
    print(json.dumps(res))
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write('# tools/eval_bench.py on one MI355X\n\n```\n' + '\n'.join(lines) + '\n```\n\nThe JSON line of the run:\n\n```\n'
                     + json.dumps(res) + '\n```\n')


if __name__ == '__main__':
    main()
