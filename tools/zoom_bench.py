#!/usr/bin/env python
"""Times zoom (K22, csrc/viewport.hip: view_render_kernel with a lens table, view_spread_kernel) at the sizes a video is run at: HIP events
around each call on the current stream, the median after warm-up, as tools/viewport_bench.py does.  64 u8 frames of 1024 x 2048
into views of 720 x 1280, cameras along a pan.  In one run:

  (1)  ops.viewport_render at 90 degrees - the yardstick, timed twice (before and after the others): its own spread
  (2)  ops.viewport_render_zoom with the same lens in every frame and no factors: what the lens table costs
  (3)  64 one-frame ops.viewport_render calls, each with its own field of view: what a user must do without K22, the baseline
       the feature is judged against; beside it ops.viewport_render_zoom with those 64 fields of view
  (4)  factors 1 .. 4 mixed over the frames in one ops.viewport_render_zoom call, against the same frames grouped by factor
       beforehand and rendered by four ops.viewport_render(.., supersample=) calls
  (5)  ops.sphere_spread on 14 x 28 and 32 x 64 maps beside ops.sphere_peak (smoothing included) on the same maps
  (6)  ViewportPilot.follow_zoom end to end beside ViewportPilot.follow on 32 x 64 maps (each holds one host synchronisation)

  python tools/zoom_bench.py [--frames 64] [--src 1024,2048] [--view 720,1280] [--reps 20] [--warmup 5]
Prints a table and one JSON line.  Nothing here is gated."""
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
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--src', default='1024,2048')
    ap.add_argument('--view', default='720,1280')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    import torch
    from cp_360_weakly_supervised_saliency_amd import ops
    from cp_360_weakly_supervised_saliency_amd.utils import hashrng
    from cp_360_weakly_supervised_saliency_amd.utils import viewport as vp

    assert torch.cuda.is_available(), "zoom_bench needs a GPU"
    F = args.frames
    H, W = (int(v) for v in args.src.split(','))
    h, w = (int(v) for v in args.view.split(','))

    # eight smooth hash textures of 1 / 8 of the size, enlarged on the device (input preparation)
    base = torch.from_numpy(hashrng.uniform(31, (8, 3, max(H // 8, 2), max(W // 8, 2)), 0.0, 255.0)).cuda()
    big = torch.nn.functional.interpolate(base, size=(H, W), mode='bilinear', align_corners=False)
    big = big.permute(0, 2, 3, 1).round().clamp(0, 255).to(torch.uint8).contiguous()
    frames = big[torch.arange(F, device='cuda') % 8].contiguous()
    del base, big

    def lonlat(lon, lat):
        lon, lat = np.deg2rad(lon), np.deg2rad(lat)
        return np.array([np.cos(lat) * np.cos(lon), np.sin(lat), np.cos(lat) * np.sin(lon)])

    # a pan that crosses the seam and climbs, 3 degrees a frame; the lens opens from 50 to 110 degrees and closes again
    centres = np.stack([lonlat(150.0 + 3.0 * f, 25.0 * np.sin(f / 10.0)) for f in range(F)])
    R = torch.from_numpy(vp.cameras(centres).astype(np.float32)).cuda()
    fovs = 80.0 - 30.0 * np.cos(2.0 * np.pi * np.arange(F) / F)
    out = torch.empty((F, h, w, 3), dtype=torch.uint8, device='cuda')
    rows = []

    def row(name, fn, note=''):
        med, lo, hi = time_ms(fn, args.reps, args.warmup)
        rows.append({'case': name, 'ms': med, 'min_ms': lo, 'max_ms': hi, 'note': note})
        return med

    # (1), (2): one lens for every frame
    lens90 = ops.viewport_lens(90.0, (h, w), device='cuda', n=F)
    yard = lambda: ops.viewport_render(frames, R, (h, w), 90.0, out=out)
    same = lambda: ops.viewport_render_zoom(frames, R, (h, w), lens90, out=out)
    assert torch.equal(yard().clone(), same())
    row('(1) viewport_render, 90 degrees', yard, 'first')
    row('(2) viewport_render_zoom, the same lens in every frame', same)
    row('(1) viewport_render, 90 degrees', yard, 'again')
    row('(2) viewport_render_zoom, the same lens in every frame', same, 'again')

    # (3): a field of view per frame
    lens = ops.viewport_lens(fovs, (h, w), device='cuda')
    ones = [(frames[n:n + 1], R[n:n + 1].contiguous(), out[n:n + 1], float(fovs[n])) for n in range(F)]

    def one_by_one():
        for fr, r, o, fov in ones:
            ops.viewport_render(fr, r, (h, w), fov, out=o)

    zoom = lambda: ops.viewport_render_zoom(frames, R, (h, w), lens, out=out)
    one_by_one()
    assert torch.equal(out.clone(), zoom())
    row('(3) %d one-frame viewport_render calls, a field of view each' % F, one_by_one, 'the baseline')
    row('(3) viewport_render_zoom, %d fields of view' % F, zoom)

    # (4): a factor per frame
    factors = 1 + np.arange(F) % 4
    ss = torch.from_numpy(factors.astype(np.int32)).cuda()
    groups = []
    for n in (1, 2, 3, 4):
        idx = torch.from_numpy(np.flatnonzero(factors == n)).cuda()
        groups.append((n, idx, frames[idx].contiguous(), R[idx].contiguous(), torch.empty((len(idx), h, w, 3), dtype=torch.uint8, device='cuda')))

    def grouped():
        for n, _, fr, r, o in groups:
            ops.viewport_render(fr, r, (h, w), 90.0, out=o, supersample=n)

    mixed = lambda: ops.viewport_render_zoom(frames, R, (h, w), lens90, out=out, supersample=ss)
    grouped()
    got = mixed()
    assert all(torch.equal(got[idx], o) for _, idx, _, _, o in groups)
    row('(4) viewport_render_zoom, factors 1 .. 4 mixed over the frames', mixed)
    row('(4) four viewport_render(.., supersample=n) calls on the frames grouped by factor', grouped, 'grouping not timed')
    del groups, got
    torch.cuda.empty_cache()

    # (5): the spread beside the peak
    for hm, wm in ((14, 28), (32, 64)):
        maps = torch.from_numpy(hashrng.uniform(32, (F, hm, wm), 0.0, 0.1).astype(np.float32)).cuda()
        px = torch.from_numpy(np.stack([vp_blob(centres[f], hm, wm, 8.0 + 17.0 * f / max(F - 1, 1)) for f in range(F)]).astype(np.float32)).cuda()
        maps = (maps + px).contiguous()
        work = ops._stab_work(0, hm, wm, maps.device)
        dirs = ops.sphere_peak(maps, 15.0, work=work)[0]
        row('(5) sphere_peak (with sphere_smooth), %d maps of %d x %d' % (F, hm, wm), lambda: ops.sphere_peak(maps, 15.0, work=work))
        row('(5) sphere_spread, %d maps of %d x %d' % (F, hm, wm), lambda: ops.sphere_spread(maps, dirs, 45.0, 0.5, work=work))

    # (6): end to end
    plain, zoomed = vp.ViewportPilot((h, w), 90.0), vp.ViewportPilot((h, w), 90.0, zoom=True)
    row('(6) ViewportPilot.follow, 32 x 64 maps', lambda: plain.follow(frames, maps))
    row('(6) ViewportPilot.follow_zoom, 32 x 64 maps', lambda: zoomed.follow_zoom(frames, maps))
    hfov = zoomed.track(maps)[1]

    print('%d u8 frames of %d x %d -> %d x %d; median of %d after %d warm-up calls (HIP events)' % (F, H, W, h, w, args.reps, args.warmup))
    print('%-88s %10s %10s %10s  %s' % ('case', 'median ms', 'min ms', 'max ms', 'note'))
    for r in rows:
        print('%-88s %10.3f %10.3f %10.3f  %s' % (r['case'], r['ms'], r['min_ms'], r['max_ms'], r['note']))
    y = [r['ms'] for r in rows if r['case'].startswith('(1)')]
    z = [r['ms'] for r in rows if r['case'].startswith('(2)')]
    print('(1) timed twice: %.3f and %.3f ms, a spread of %.2f %%; (2) / (1) = %.3f and %.3f' % (y[0], y[1], 100.0 * abs(y[1] - y[0]) / min(y),
                                                                                              z[0] / y[0], z[1] / y[1]))
    print('(3) one launch over the one-frame calls: %.2f x' % (rows[4]['ms'] / rows[5]['ms']))
    print('(4) mixed / grouped = %.3f' % (rows[6]['ms'] / rows[7]['ms']))
    print('(6) the fields of view of follow_zoom: %.1f .. %.1f degrees' % (float(hfov.min()), float(hfov.max())))
    print(json.dumps({'tool': 'zoom_bench', 'frames': F, 'src': [H, W], 'view': [h, w], 'rows': rows}))


def vp_blob(centre, hm, wm, sigma_deg):
    """exp(-theta^2 / (2 sigma^2)) of the angle to `centre` on the hm x wm map, float64."""
    tt = np.pi * ((2.0 * np.arange(wm) + 1.0) / wm - 1.0)
    tp = np.pi * 0.5 * (1.0 - (2.0 * np.arange(hm) + 1.0) / hm)
    p = np.stack([np.cos(tp)[:, None] * np.cos(tt)[None, :], np.broadcast_to(np.sin(tp)[:, None], (hm, wm)),
                  np.cos(tp)[:, None] * np.sin(tt)[None, :]], -1)
    theta = np.arccos(np.clip(p @ (centre / np.linalg.norm(centre)), -1.0, 1.0))
    return np.exp(-0.5 * (theta / np.deg2rad(sigma_deg)) ** 2)


if __name__ == '__main__':
    main()
