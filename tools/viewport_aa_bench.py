#!/usr/bin/env python
"""Times the anti-aliased view (K21, csrc/viewport.hip: view_render_kernel with a factor and the canvas kernel with a factor per
tile) at the sizes a video is run at: HIP events around each call on the current stream, the median after warm-up, as tools/viewport_bench.py
does.  64 u8 frames of 2048 x 4096, cameras along a pan.

  cases      720 x 1280 at 90 degrees (supersample_for: 2) and at 120 degrees (2); a canvas of two 360 x 640 tiles and a gutter of 8
             (3); and n = 1 .. 4 at the first shape
  fused      ops.viewport_render(.., supersample=n) / ops.viewport_render_multi(.., supersample=n): one launch
  (a)        the same call without supersample: what anti-aliasing costs - reported, not gated
  (b)        what a caller can write without K21: the view (n h, n w) with one sample per pixel - for the canvas, tiles and gutter n
             times as large -, then torch.nn.functional.avg_pool2d and the rounding in torch.  It rounds every sample to u8 before
             the mean, so it may differ from the fused view by one level; the tool counts the values that do
Every case is timed as (a), (b), fused, (a), (b), fused: alternating pairs, and the ratio fused / (b) of each pair is printed.

  python tools/viewport_aa_bench.py [--frames 64] [--src 2048,4096] [--view 720,1280] [--tile 360,640] [--reps 20] [--warmup 5]
Prints a table and one JSON line."""
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--src', default='2048,4096')
    ap.add_argument('--view', default='720,1280')
    ap.add_argument('--tile', default='360,640')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    import torch
    from cp_360_weakly_supervised_saliency_amd import ops
    from cp_360_weakly_supervised_saliency_amd.utils import hashrng
    from cp_360_weakly_supervised_saliency_amd.utils import viewport as vp

    assert torch.cuda.is_available(), "viewport_aa_bench needs a GPU"
    F = args.frames
    H, W = (int(v) for v in args.src.split(','))
    h, w = (int(v) for v in args.view.split(','))
    th, tw = (int(v) for v in args.tile.split(','))

    # eight smooth hash textures of 1 / 8 of the size, enlarged on the device (input preparation)
    base = torch.from_numpy(hashrng.uniform(31, (8, 3, max(H // 8, 2), max(W // 8, 2)), 0.0, 255.0)).cuda()
    big = torch.nn.functional.interpolate(base, size=(H, W), mode='bilinear', align_corners=False)
    big = big.permute(0, 2, 3, 1).round().clamp(0, 255).to(torch.uint8).contiguous()
    frames = big[torch.arange(F, device='cuda') % 8].contiguous()
    del base, big

    def lonlat(lon, lat):
        lon, lat = np.deg2rad(lon), np.deg2rad(lat)
        return np.array([np.cos(lat) * np.cos(lon), np.sin(lat), np.cos(lat) * np.sin(lon)])

    # two cameras 110 degrees apart along a pan that crosses the seam and climbs: 3 degrees a frame
    t = 150.0 + 3.0 * np.arange(F)
    paths = [np.stack([lonlat(t[f] + off, 25.0 * np.sin(f / 10.0)) for f in range(F)]) for off in (0.0, 110.0)]
    R2 = torch.from_numpy(np.stack([vp.cameras(p) for p in paths], 1).astype(np.float32)).cuda()
    R = R2[:, 0].contiguous()

    def pooled(fine, n):
        """The n x n mean of a u8 view [F, n h, n w, 3] in torch, rounded half to even: [F, h, w, 3] u8."""
        x = torch.nn.functional.avg_pool2d(fine.permute(0, 3, 1, 2).float(), n)
        return x.round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()

    def single(hfov, n):
        out = torch.empty((F, h, w, 3), dtype=torch.uint8, device='cuda')
        fine = torch.empty((F, n * h, n * w, 3), dtype=torch.uint8, device='cuda')
        fused = lambda: ops.viewport_render(frames, R, (h, w), hfov, out=out, supersample=n)
        plain = lambda: ops.viewport_render(frames, R, (h, w), hfov, out=out)
        yard = lambda: pooled(ops.viewport_render(frames, R, (n * h, n * w), hfov, out=fine), n)
        return fused, plain, yard, F * h * w

    def canvas(hfov, n, gutter=8):
        tiles, canvas_hw = vp.split_layout(2, (th, tw), gutter)
        tiles_n, canvas_n = vp.split_layout(2, (n * th, n * tw), n * gutter)
        out = torch.empty((F,) + canvas_hw + (3,), dtype=torch.uint8, device='cuda')
        fine = torch.empty((F,) + canvas_n + (3,), dtype=torch.uint8, device='cuda')
        fused = lambda: ops.viewport_render_multi(frames, R2, tiles, hfov, canvas_hw, out=out, supersample=n)
        plain = lambda: ops.viewport_render_multi(frames, R2, tiles, hfov, canvas_hw, out=out)
        yard = lambda: pooled(ops.viewport_render_multi(frames, R2, tiles_n, hfov, canvas_n, out=fine), n)
        return fused, plain, yard, F * canvas_hw[0] * canvas_hw[1]

    auto = vp.supersample_for((H, W), (h, w), 90.0), vp.supersample_for((H, W), (h, w), 120.0), vp.supersample_for((H, W), (th, tw), 90.0)
    cases = [('%dx%d -> %dx%d, 90 degrees, auto' % (H, W, h, w), single, 90.0, auto[0]),
             ('%dx%d -> %dx%d, 120 degrees, auto' % (H, W, h, w), single, 120.0, auto[1]),
             ('%dx%d -> canvas of 2 x %dx%d, 90 degrees, auto' % (H, W, th, tw), canvas, 90.0, auto[2])]
    cases += [('%dx%d -> %dx%d, 90 degrees' % (H, W, h, w), single, 90.0, n) for n in (1, 2, 3, 4)]
    rows = []
    for name, make, hfov, n in cases:
        fused, plain, yard, px = make(hfov, n)
        timed = [time_ms(fn, args.reps, args.warmup) for fn in (plain, yard, fused, plain, yard, fused)]
        got, want = fused().clone(), yard()
        diff = (got.to(torch.int16) - want.to(torch.int16)).abs()
        assert int(diff.max()) <= 1, "the fused view and the yardstick differ by more than one level"
        rows.append({'case': name, 'n': n, 'out_pixels': px, 'samples': px * n * n,
                     'a_ms': [timed[0][0], timed[3][0]], 'b_ms': [timed[1][0], timed[4][0]], 'fused_ms': [timed[2][0], timed[5][0]],
                     'fused_min_ms': [timed[2][1], timed[5][1]],
                     'fused_over_a': [timed[2][0] / timed[0][0], timed[5][0] / timed[3][0]],
                     'fused_over_b': [timed[2][0] / timed[1][0], timed[5][0] / timed[4][0]],
                     'ns_per_sample': timed[2][0] * 1e6 / (px * n * n),
                     'values_off_by_one_from_b': int(diff.sum()), 'values': int(diff.numel())})
        del fused, plain, yard, got, want, diff
        torch.cuda.empty_cache()

    print('%d u8 frames; median of %d after %d warm-up calls (HIP events); every case timed (a), (b), fused, (a), (b), fused'
          % (F, args.reps, args.warmup))
    print('%-58s %2s %15s %17s %15s %13s %13s %10s %12s' % ('case', 'n', '(a) plain ms', '(b) yardstick ms', 'fused ms', 'fused / (a)',
                                                         'fused / (b)', 'ns/sample', 'off by one'))
    pair = lambda v, f: '%s, %s' % (f % v[0], f % v[1])
    for r in rows:
        print('%-58s %2d %15s %17s %15s %13s %13s %10.4f %12s' % (
            r['case'], r['n'], pair(r['a_ms'], '%.3f'), pair(r['b_ms'], '%.3f'), pair(r['fused_ms'], '%.3f'), pair(r['fused_over_a'], '%.2f'),
            pair(r['fused_over_b'], '%.2f'), r['ns_per_sample'], '%.2e' % (r['values_off_by_one_from_b'] / r['values'])))
    slower = [r['case'] + ' n=%d' % r['n'] for r in rows if r['n'] > 1 and max(r['fused_over_b']) > 1.0]
    print('fused slower than (b) in a pair: %s' % (slower or 'no case'))
    print(json.dumps({'tool': 'viewport_aa_bench', 'frames': F, 'src': [H, W], 'view': [h, w], 'tile': [th, tw], 'rows': rows,
                      'fused_slower_than_b': slower}))


if __name__ == '__main__':
    main()
