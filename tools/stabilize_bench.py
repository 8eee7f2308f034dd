#!/usr/bin/env python
"""Times the 360-degree stabilisation kernels (K11, csrc/stabilize.hip) at the driver's 480 x 960 for F = 1, 16, 64 pairs or
frames per call: HIP events around each call on the current stream, the median after warm-up, next to the bytes the kernels
must move and the time the HBM read ceiling the project measured (6.0 - 6.4 TB/s, tools/read_ceiling.hip) allows for them.

Bytes model (compulsory traffic only; the tables, the partials and the gathers' re-reads are left to the caches):
  fit      reads the flow once per iteration: iters x 8 H W bytes per pair (8 x 3.7 MB at 480 x 960); 2 + 2 iters launches
  rotate   reads and writes each frame once: 2 H W C bytes (u8 RGB) or 8 H W C bytes (f32) per frame; 2 launches
  flow     writes 8 H W bytes per rotation; 2 launches

  python tools/stabilize_bench.py [--counts 1,16,64] [--hw 480,960] [--reps 20] [--warmup 5] [--iters 8] [--driver F]
--driver F also times Stabilizer.stabilize and Stabilizer.from_frames on F + 1 u8 frames (Farneback, fit, the host
composition of the rotations with its synchronisation, the re-rendering; from_frames adds the second Farneback).
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
    from cp_360_weakly_supervised_saliency_amd.utils import synth
    from cp_360_weakly_supervised_saliency_amd.utils.stabilize import Stabilizer
    from tests import stabilize_restate as sr

    assert torch.cuda.is_available(), "stabilize_bench needs a GPU"
    H, W = (int(v) for v in args.hw.split(','))
    counts = [int(v) for v in args.counts.split(',')]
    px = 2 * np.pi / W
    # nine distinct small rotations (1 - 3 px-equivalents), their flows from K11b plus a moving rectangle, one u8 frame each
    Rs = np.stack([sr.rot((0.3 + 0.1 * i, 0.8, -0.5 + 0.1 * i), (1.0 + 0.25 * i) * px) for i in range(9)]).astype(np.float32)
    flows9 = ops.rotation_flow(torch.from_numpy(Rs).cuda(), H, W)
    flows9[:, H // 3:2 * H // 3, W // 4:W // 2] += 2.0
    frames9 = torch.from_numpy(np.stack([synth.frame_u8(40 + i, H, W) for i in range(9)])).cuda()
    rows = []
    for n in counts:
        idx = torch.arange(n, device='cuda') % 9
        flow, frames, R = flows9[idx].contiguous(), frames9[idx].contiguous(), torch.from_numpy(Rs).cuda()[idx].contiguous()
        frames_f = frames.float()
        work = ops._stab_work(n, H, W, flow.device)
        out_u8, out_f = torch.empty_like(frames), torch.empty_like(frames_f)
        ms, fastest = time_ms(lambda: ops.rotation_fit(flow, args.iters, work=work), args.reps, args.warmup)
        rows.append(row('fit (%d iterations)' % args.iters, n, ms, fastest, args.iters * 8.0 * H * W * n, 2 + 2 * args.iters))
        ms, fastest = time_ms(lambda: ops.equirect_rotate(frames, R, out=out_u8, work=work), args.reps, args.warmup)
        rows.append(row('rotate u8 RGB', n, ms, fastest, 2.0 * 3 * H * W * n, 2))
        ms, fastest = time_ms(lambda: ops.equirect_rotate(frames_f, R, out=out_f, work=work), args.reps, args.warmup)
        rows.append(row('rotate f32 x 3', n, ms, fastest, 8.0 * 3 * H * W * n, 2))
        ms, fastest = time_ms(lambda: ops.rotation_flow(R, H, W, work=work), args.reps, args.warmup)
        rows.append(row('rotation flow', n, ms, fastest, 8.0 * H * W * n, 2))
    print('%d x %d; HBM bound at %.1f - %.1f TB/s' % ((H, W) + READ_CEILING_TBPS))
    print('%-22s %6s %12s %12s %12s %12s %16s %9s' % ('kernel', 'count', 'ms / call', 'us / item', 'MB / item', 'model TB/s',
                                                       'HBM bound us/item', 'x bound'))
    for r in rows:
        print('%-22s %6d %12.3f %12.2f %12.2f %12.3f %8.2f-%-7.2f %9.1f' % (r['kernel'], r['count'], r['ms_per_call'], r['us_per_item'],
                                                                           r['model_MB_per_item'], r['model_TBps'],
                                                                           r['hbm_bound_us_per_item'][0], r['hbm_bound_us_per_item'][1],
                                                                           r['x_hbm_bound']))
    result = {'tool': 'stabilize_bench', 'hw': [H, W], 'iters': args.iters, 'rows': rows}
    if args.driver:
        F = args.driver
        st = Stabilizer((H, W), iters=args.iters)
        video = frames9[torch.arange(F + 1, device='cuda') % 9].contiguous()
        result['driver'] = {'frames': F + 1}
        for name, fn in (('farneback alone', lambda: st.flow.from_frames(video, res=(W, H))), ('rotations', lambda: st.rotations(video)),
                         ('stabilize', lambda: st.stabilize(video)), ('from_frames', lambda: st.from_frames(video))):
            ms, _ = time_ms(fn, args.reps, args.warmup)
            result['driver'][name] = {'ms_per_call': ms, 'ms_per_pair': ms / F}
            print('driver, %d frames: %-16s %9.3f ms / call, %8.3f ms / pair' % (F + 1, name, ms, ms / F))
    print(json.dumps(result))


if __name__ == '__main__':
    main()
