#!/usr/bin/env python
"""Times the Farneback optical flow (K10, utils/optical_flow.py: FarnebackFlow) at the reference's 480 x 960 for F = 1, 16,
64 pairs per call: HIP events around each call on the current stream, the median after warm-up, as ms per pair - next to the
bytes the kernels must move per pair by the model below and the HBM rate that time corresponds to.

Bytes model (compulsory traffic only: every tensor read and written once per kernel that touches it, halos and the gathers'
re-reads left to the caches), in floats, n_k = pixels of level k, n = n_0, per level:
  per FRAME   pyramid: horizontal blur reads n and writes n, the vertical blur + resize reads n and writes n_k  (3 n + n_k)
              expansion: reads n_k, writes 5 n_k                                                              (6 n_k)
  per PAIR    incoming flow: zero fill 2 n_k at the coarsest level, else read 2 n_k+1 and write 2 n_k
              per iteration: matrices reads flow 2 n_k, R of both frames 10 n_k, writes M 5 n_k              (17 n_k)
                             blur-and-solve reads M 5 n_k, writes flow 2 n_k                                  (7 n_k)
A call of F pairs expands F + 1 frames, so the per-frame part counts (F + 1) / F times per pair.

  python tools/optflow_bench.py [--pairs 1,16,64] [--hw 480,960] [--reps 20] [--restate] [--stages F]
--stages F also times every stage alone through its entry point at every level's size for F pairs (ms per launch and the
rate of that launch's compulsory bytes); --restate also times the float64 numpy restatement (tests/farneback_restate.py) of one pair on this machine's CPU, for scale.
Prints a table and one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def model_bytes_per_pair(geometry, F, iterations):
    n = geometry[0][0] * geometry[0][1]
    frame = pair = 0.0
    for k, (h, w, _, _) in enumerate(geometry):
        nk = h * w
        frame += 3 * n + nk + 6 * nk
        if k == len(geometry) - 1:
            pair += 2 * nk
        else:
            pair += 2 * geometry[k + 1][0] * geometry[k + 1][1] + 2 * nk
        pair += iterations * (17 + 7) * nk
    return 4.0 * (frame * (F + 1) / F + pair)


def launches_per_call(geometry, iterations):
    return len(geometry) * (2 + 1 + 1 + 2 * iterations)


def synthetic_gray(n_frames, hw, seed=5):
    """A drifting smooth texture plus noise, rounded to u8 levels: what the gray conversion delivers."""
    h, w = hw
    rs = np.random.RandomState(seed)
    kx, ky, ph = rs.uniform(-0.35, 0.35, 24), rs.uniform(-0.35, 0.35, 24), rs.uniform(0, 2 * np.pi, 24)
    y, x = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing='ij')
    base = [np.float32(a) for a in (1.3, 0.7)]
    out = np.empty((n_frames, h, w), np.float32)
    for t in range(n_frames):
        img = np.zeros((h, w), np.float32)
        for i in range(24):
            img += np.sin(np.float32(kx[i]) * (x + base[0] * t) + np.float32(ky[i]) * (y + base[1] * t) + np.float32(ph[i]))
        out[t] = np.clip(np.rint(127.5 + 12.0 * img + rs.normal(0, 1.0, (h, w))), 0, 255)
    return out


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


def stage_rows(ff, gray, F, reps, warmup):
    """Each stage alone at every level: (stage, level, ms per launch, compulsory MB, TB/s)."""
    import torch
    from cp_360_weakly_supervised_saliency_amd import ops
    H, W = ff.hw
    n = H * W
    rows = []
    for k, (h, w, ksz, sigma) in enumerate(ff.geometry):
        nk = h * w
        img = ops.optflow_pyr_level(gray, ksz, sigma, h, w)
        R = ops.optflow_poly_exp(img, ff.poly_n, ff.poly_sigma)
        flow = torch.zeros(F, h, w, 2, device='cuda')
        M = ops.optflow_matrices(R[:-1], R[1:], flow)
        flow = ops.optflow_blur_solve(M, ff.winsize)
        cases = [('pyr_level (2 launches)', lambda: ops.optflow_pyr_level(gray, ksz, sigma, h, w), (F + 1) * (3 * n + nk)),
                 ('poly_exp', lambda: ops.optflow_poly_exp(img, ff.poly_n, ff.poly_sigma), (F + 1) * 6 * nk),
                 ('matrices', lambda: ops.optflow_matrices(R[:-1], R[1:], flow), F * 17 * nk),
                 ('blur_solve', lambda: ops.optflow_blur_solve(M, ff.winsize), F * 7 * nk)]
        if k > 0:
            fh, fw = ff.geometry[k - 1][:2]
            cases.append(('flow_upsample (to level %d)' % (k - 1), lambda: ops.optflow_flow_upsample(flow, fh, fw, 2.0),
                          F * (2 * nk + 2 * fh * fw)))
        for name, fn, floats in cases:
            ms, _ = time_ms(fn, reps, warmup)              # includes the wrapper's output allocation (cached by torch)
            rows.append({'stage': name, 'level': k, 'hw': [h, w], 'ms': ms, 'model_MB': 4e-6 * floats,
                         'model_TBps': 4.0 * floats / (ms * 1e-3) / 1e12})
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--pairs', default='1,16,64')
    ap.add_argument('--hw', default='480,960')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--restate', action='store_true')
    ap.add_argument('--stages', type=int, default=0)
    args = ap.parse_args()
    import torch
    from cp_360_weakly_supervised_saliency_amd.utils.optical_flow import FarnebackFlow

    hw = tuple(int(v) for v in args.hw.split(','))
    pairs = [int(v) for v in args.pairs.split(',')]
    assert torch.cuda.is_available(), "optflow_bench needs a GPU"
    ff = FarnebackFlow(hw)
    distinct = synthetic_gray(min(max(pairs) + 1, 9), hw)
    rows = []
    for F in pairs:
        gray = torch.from_numpy(distinct[np.arange(F + 1) % distinct.shape[0]]).cuda()
        out = torch.empty((F,) + hw + (2,), dtype=torch.float32, device='cuda')
        ms, fastest = time_ms(lambda: ff(gray, out), args.reps, args.warmup)
        mb = model_bytes_per_pair(ff.geometry, F, ff.iterations)
        rows.append({'pairs': F, 'ms_per_call': ms, 'ms_per_pair': ms / F, 'min_ms_per_pair': fastest / F,
                     'model_MB_per_pair': mb / 1e6, 'model_TBps': mb / (ms / F * 1e-3) / 1e12,
                     'launches_per_call': launches_per_call(ff.geometry, ff.iterations),
                     'workspace_MB': ff.work_bytes(F) / 1e6})
    print('%dx%d, %d levels, winsize %d, %d iterations, poly_n %d' % (hw + (len(ff.geometry), ff.winsize, ff.iterations, ff.poly_n)))
    print('%6s %12s %12s %14s %12s %10s' % ('pairs', 'ms / call', 'ms / pair', 'model MB/pair', 'model TB/s', 'launches'))
    for r in rows:
        print('%6d %12.3f %12.4f %14.1f %12.3f %10d' % (r['pairs'], r['ms_per_call'], r['ms_per_pair'], r['model_MB_per_pair'],
                                                        r['model_TBps'], r['launches_per_call']))
    result = {'tool': 'optflow_bench', 'hw': list(hw), 'rows': rows}
    if args.stages:
        F = args.stages
        gray = torch.from_numpy(distinct[np.arange(F + 1) % distinct.shape[0]]).cuda()
        result['stages'] = stage_rows(ff, gray, F, args.reps, args.warmup)
        print('stages alone, %d pairs:' % F)
        for r in result['stages']:
            print('  level %d %4dx%-4d %-30s %8.3f ms %9.1f MB %7.3f TB/s' % (r['level'], r['hw'][0], r['hw'][1], r['stage'],
                                                                              r['ms'], r['model_MB'], r['model_TBps']))
    if args.restate:
        from tests import farneback_restate as fb
        t0 = time.perf_counter()
        fb.farneback(distinct[:2])
        result['restate_f64_cpu_s_per_pair'] = time.perf_counter() - t0
        print('float64 numpy restatement on this CPU: %.2f s per pair' % result['restate_f64_cpu_s_per_pair'])
    print(json.dumps(result))


if __name__ == '__main__':
    main()
