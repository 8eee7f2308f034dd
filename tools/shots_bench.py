#!/usr/bin/env python
"""Times the shot-signature kernel (K13, csrc/shots.hip) for 1, 16 and 64 frames at 480 x 960, 1024 x 2048 and 2048 x 4096 on two
inputs - a blurred texture and a constant frame, the worst case for contention on a histogram bin -: HIP events around each
call on the current stream, the median after warm-up, next to the bytes the kernel must move and the time the HBM read ceiling
the project measured (6.0 - 6.4 TB/s, profiles/r05_read_ceiling.md) allows for them.

Bytes model (compulsory traffic only): every frame is read once, 3 H W bytes; the weight table (4 H bytes, cached), the u32
partials (768 bytes per workgroup, written and read once) and the signatures (1536 bytes per frame) are left out.  Two launches.
A batch of 64 frames of 480 x 960 is 88 MB: it fits the 256 MiB Infinity Cache, so repeated calls on it need not reach HBM; 64 frames
of 1024 x 2048 (403 MB) and of 2048 x 4096 (1.6 GB) do not fit.

  python tools/shots_bench.py [--counts 1,16,64] [--sizes 480x960,1024x2048,2048x4096] [--reps 20] [--warmup 5] [--driver 65]
                              [--out profiles/shots_bench.md]
--driver F also times ShotDetector.cuts on F frames of every size (signatures, the distances in torch, the copy of F - 1 values
to the host with its synchronisation, find_cuts).  Prints a table and one JSON line; --out writes both as markdown."""
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


def texture_u8(H, W):
    """One blurred hash texture, u8 [H, W, 3] (utils/synth.py's box blur, 9 taps, stretched to the full range)."""
    from cp_360_weakly_supervised_saliency_amd.utils import hashrng, synth
    t = synth._box_blur(hashrng.uniform(77, (H, W, 3), 0.0, 1.0), 9)
    t = (t - t.min()) / float(t.max() - t.min())
    return np.rint(255.0 * t).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--counts', default='1,16,64')
    ap.add_argument('--sizes', default='480x960,1024x2048,2048x4096')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--driver', type=int, default=65)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from cp_360_weakly_supervised_saliency_amd import ops
    from cp_360_weakly_supervised_saliency_amd.utils.shots import ShotDetector

    assert torch.cuda.is_available(), "shots_bench needs a GPU"
    counts = [int(v) for v in args.counts.split(',')]
    sizes = [tuple(int(v) for v in s.split('x')) for s in args.sizes.split(',')]
    rows, driver = [], {}
    for H, W in sizes:
        base = torch.from_numpy(texture_u8(H, W)).cuda()
        weights = ops.shot_weights(H, base.device)
        T = W * ops.shot_weights_host(H)[1]
        for n in counts:
            # frame k of the texture batch is the texture rolled by 37 k columns: distinct bytes, the same signature
            tex = torch.stack([torch.roll(base, 37 * k, dims=1) for k in range(n)]).contiguous()
            const = torch.full_like(tex, 200)
            work = ops._shot_work(n, H, W, base.device)
            per = {}
            for name, frames in (('texture', tex), ('constant', const)):
                sig = ops.shot_signatures(frames, work=work, weights=weights)
                assert bool((sig.sum(dim=2) == T).all()), "signature does not sum to T"
                ms, fastest = time_ms(lambda: ops.shot_signatures(frames, work=work, weights=weights), args.reps, args.warmup)
                nbytes = 3.0 * H * W * n
                bound_us = [nbytes / (c * 1e12) * 1e6 for c in READ_CEILING_TBPS[::-1]]
                per[name] = ms
                rows.append({'size': '%dx%d' % (H, W), 'input': name, 'frames': n, 'ms_per_call': ms, 'us_per_frame': 1e3 * ms / n,
                             'min_us_per_frame': 1e3 * fastest / n, 'model_MB_per_frame': nbytes / n / 1e6,
                             'model_TBps': nbytes / (ms * 1e-3) / 1e12, 'hbm_bound_us_per_frame': [b / n for b in bound_us],
                             'x_hbm_bound': ms * 1e3 / bound_us[1], 'launches': 2})
            rows[-1]['constant_over_texture'] = per['constant'] / per['texture']
            del tex, const
        if args.driver:
            F = args.driver
            video = torch.stack([torch.roll(base, 37 * k, dims=1) for k in range(F)]).contiguous()
            video[F // 2:] //= 2                                       # one cut in the middle: the second half is darker
            det = ShotDetector(thr=0.25, ratio=3.0, radius=8)
            assert det.cuts(video) == [F // 2], det.cuts(video)
            ms, _ = time_ms(lambda: det.cuts(video), args.reps, args.warmup)
            driver['%dx%d' % (H, W)] = {'frames': F, 'ms_per_call': ms, 'ms_per_frame': ms / F}
            del video
    lines = ['HBM bound at %.1f - %.1f TB/s; median of %d after %d warm-up calls (HIP events)' % (READ_CEILING_TBPS + (args.reps, args.warmup)),
             '%-10s %-9s %6s %10s %11s %10s %11s %17s %8s %12s' % ('size', 'input', 'frames', 'ms / call', 'us / frame', 'MB / frame',
                                                                   'model TB/s', 'HBM bound us/frame', 'x bound', 'const / tex')]
    for r in rows:
        lines.append('%-10s %-9s %6d %10.3f %11.2f %10.2f %11.3f %8.2f-%-8.2f %8.2f %12s'
                     % (r['size'], r['input'], r['frames'], r['ms_per_call'], r['us_per_frame'], r['model_MB_per_frame'], r['model_TBps'],
                        r['hbm_bound_us_per_frame'][0], r['hbm_bound_us_per_frame'][1], r['x_hbm_bound'],
                        '%.2f' % r['constant_over_texture'] if 'constant_over_texture' in r else ''))
    for size, d in driver.items():
        lines.append('ShotDetector.cuts, %d frames of %s: %.3f ms / call, %.4f ms / frame' % (d['frames'], size, d['ms_per_call'], d['ms_per_frame']))
    print('\n'.join(lines))
    result = {'tool': 'shots_bench', 'reps': args.reps, 'warmup': args.warmup, 'rows': rows, 'driver': driver}
    print(json.dumps(result))
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write('# tools/shots_bench.py on one MI355X (HIP events, median of %d after %d warm-up calls)\n\n```\n' % (args.reps, args.warmup))
            fh.write('\n'.join(lines) + '\n```\n\nThe JSON line of the run:\n\n```\n' + json.dumps(result) + '\n```\n')


if __name__ == '__main__':
    main()
