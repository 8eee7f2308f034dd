#!/usr/bin/env python
"""Times the ego-motion kernels (K23, csrc/egomotion.hip) at the driver's 480 x 960 for F = 1, 16, 64 pairs per call: HIP events
around each call on the current stream, the median after warm-up, next to the bytes the kernels must move and the time the HBM
read ceiling the project measured (6.0 - 6.4 TB/s, profiles/r05_read_ceiling.md) allows for them.  The yardstick beside the fit is
K11's rotation fit (csrc/stabilize.hip) on the same flows in the same run: both re-read the flow once per iteration.

Bytes model (compulsory traffic only; the tables and the partials are left to the caches):
  ego fit       reads the flow once per iteration: iters x 8 H W bytes per pair; 2 + 2 iters launches (from a given R0)
  K11 fit       the same bytes; 2 + 2 iters launches
  residual      reads the flow and writes the residual: 16 H W bytes per pair (+ 4 H W with mag); 2 launches

  python tools/egomotion_bench.py [--counts 1,16,64] [--hw 480,960] [--reps 20] [--warmup 5] [--iters 8] [--driver F]
--driver F also times Stabilizer.from_frames, .egomotion and .independent_flow on F + 1 u8 frames of a travelling camera.
Prints a table and one JSON line."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

READ_CEILING_TBPS = (6.0, 6.4)


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


def row(kernel, count, ms, fastest, nbytes, launches):
    bound_us = [nbytes / (c * 1e12) * 1e6 for c in READ_CEILING_TBPS[::-1]]
    return {'kernel': kernel, 'count': count, 'ms_per_call': ms, 'us_per_item': 1e3 * ms / count, 'min_us_per_item': 1e3 * fastest / count,
            'model_MB_per_item': nbytes / count / 1e6, 'model_TBps': nbytes / (ms * 1e-3) / 1e12,
            'hbm_bound_us_per_item': [b / count for b in bound_us], 'x_hbm_bound': ms * 1e3 / bound_us[1], 'launches': launches}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--counts', default='1,16,64')
    ap.add_argument('--hw', default='480,960')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=8)
    ap.add_argument('--driver', type=int, default=0)
    args = ap.parse_args()
    import torch
    from cp_360_weakly_supervised_saliency_amd import ops
    from cp_360_weakly_supervised_saliency_amd.utils.stabilize import Stabilizer
    from tests import egomotion_restate as er

    assert torch.cuda.is_available(), "egomotion_bench needs a GPU"
    H, W = (int(v) for v in args.hw.split(','))
    counts = [int(v) for v in args.counts.split(',')]
    # four distinct scene flows: translations of 0.05 .. 0.2 along different directions, 0.05 px of noise, the mover
    dirs = [er.E_TRUE, [-0.5, 0.3, 0.81], [0.1, -0.6, -0.79], [0.9, 0.1, -0.4]]
    flows4 = torch.from_numpy(np.stack([er.scene_flow(H, W, 0.05 * (i + 1), e_true=np.asarray(d) / np.linalg.norm(d), noise_px=0.05,
                                                      seed=500 + i, mover=(2.5, 0.0))[0] for i, d in enumerate(dirs)]).astype(np.float32)).cuda()
    rows = []
    for n in counts:
        flow = flows4[torch.arange(n, device='cuda') % 4].contiguous()
        work = ops._ego_work(n, H, W, flow.device)
        R0 = ops.rotation_fit(flow, args.iters, work=work)[0]
        R, e, diag = ops.egomotion_fit(flow, R0=R0, iters=args.iters, work=work)
        assert bool((diag[:, 7] == 0).all()), "the bench flows must pass the gate"
        out = torch.empty_like(flow)
        ms, fastest = time_ms(lambda: ops.rotation_fit(flow, args.iters, work=work), args.reps, args.warmup)
        rows.append(row('K11 fit (%d iterations)' % args.iters, n, ms, fastest, args.iters * 8.0 * H * W * n, 2 + 2 * args.iters))
        k11 = ms
        ms, fastest = time_ms(lambda: ops.egomotion_fit(flow, R0=R0, iters=args.iters, work=work), args.reps, args.warmup)
        rows.append(row('ego fit (%d iterations)' % args.iters, n, ms, fastest, args.iters * 8.0 * H * W * n, 2 + 2 * args.iters))
        rows[-1]['x_k11_fit'] = ms / k11
        ms, fastest = time_ms(lambda: ops.egomotion_residual(flow, R, e, out=out, work=work), args.reps, args.warmup)
        rows.append(row('residual', n, ms, fastest, 16.0 * H * W * n, 2))
        ms, fastest = time_ms(lambda: ops.egomotion_residual(flow, R, e, out=out, want_mag=True, work=work), args.reps, args.warmup)
        rows.append(row('residual + mag', n, ms, fastest, 20.0 * H * W * n, 2))
    print('%d x %d; HBM bound at %.1f - %.1f TB/s' % ((H, W) + READ_CEILING_TBPS))
    print('%-24s %6s %12s %12s %12s %12s %16s %9s %9s' % ('kernel', 'count', 'ms / call', 'us / item', 'MB / item', 'model TB/s',
                                                         'HBM bound us/item', 'x bound', 'x K11 fit'))
    for r in rows:
        print('%-24s %6d %12.3f %12.2f %12.2f %12.3f %8.2f-%-7.2f %9.1f %9s' % (
            r['kernel'], r['count'], r['ms_per_call'], r['us_per_item'], r['model_MB_per_item'], r['model_TBps'],
            r['hbm_bound_us_per_item'][0], r['hbm_bound_us_per_item'][1], r['x_hbm_bound'],
            '%.2f' % r['x_k11_fit'] if 'x_k11_fit' in r else ''))
    result = {'tool': 'egomotion_bench', 'hw': [H, W], 'iters': args.iters, 'rows': rows}
    if args.driver:
        F = args.driver
        st = Stabilizer((H, W), iters=args.iters)
        video = torch.from_numpy(er.render_travelling((H, W), F + 1, 0.05, detail=W / 128.0)[0]).cuda()
        result['driver'] = {'frames': F + 1}
        for name, fn in (('from_frames', lambda: st.from_frames(video)), ('egomotion', lambda: st.egomotion(video)),
                         ('independent_flow', lambda: st.independent_flow(video))):
            ms, _ = time_ms(fn, args.reps, args.warmup)
            result['driver'][name] = {'ms_per_call': ms, 'ms_per_pair': ms / F}
            print('driver, %d frames: %-18s %9.3f ms / call, %8.3f ms / pair' % (F + 1, name, ms, ms / F))
        gated = int((st.independent_flow(video)[2][:, 7] != 0).sum())
        result['driver']['gated_pairs'] = gated
        print('driver, %d frames: %d of %d pairs gated or singular' % (F + 1, gated, F))
    print(json.dumps(result))


if __name__ == '__main__':
    main()
