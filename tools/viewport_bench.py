#!/usr/bin/env python
"""Times the viewport pilot's kernels (K12, csrc/viewport.hip) at the sizes a video is run at: HIP events around each call on the
current stream, the median after warm-up, the shader clock the chip holds under a bare MFMA loop stated next to them
(ops.held_clock_ghz), and for each kernel ns per output pixel and GB/s over the bytes the algorithm must move.

  render    64 u8 frames of 1024 x 2048 -> 720 x 1280 views, 90 degrees, cameras along a pan
            bytes = the views written + the source footprint of every view (the panorama pixels inside it, counted with
            cp360_view_outline itself: a border wider than the view paints its whole area)
  rotate    the yardstick: cp360_stab_rotate (K11c, the parent's kernel: the same sampler and the same atan2f / asinf per pixel)
            on 64 u8 frames of 720 x 1280, i.e. the same number of output pixels; bytes = frames read + written
  outline   64 u8 panoramas of 1024 x 2048, in place (bytes = the border pixels written) and out of place (read + written)
  smooth    64 maps of 14 x 28 and of 32 x 64: all pairs, P^2 terms per map; bytes = maps read + written
  peak      the same maps; bytes = smoothed + raw maps read
  path      K16, ops.sphere_path on the same maps (smoothed, every frame's gain 4096 / its peak): one sequence of F frames (one
            workgroup on one CU, F dependent steps) and 64 sequences of F frames each; bytes = maps read + back-pointers written
  refine    K16c, ops.sphere_refine about the path's pixels; bytes = raw maps read
  follow    ViewportPilot.follow end to end: smooth, peak, the copy of the peaks to the host with its synchronisation, the path
            on the host, the copy back, render
  .path     ViewportPilot.path alone with both planners: 'peak' is the yardstick of 'viterbi' in the same run

  python tools/viewport_bench.py [--frames 64] [--src 1024,2048] [--view 720,1280] [--hfov 90] [--reps 20] [--warmup 5]
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


def row(kernel, ms, fastest, out_px, nbytes, launches):
    return {'kernel': kernel, 'ms_per_call': ms, 'min_ms_per_call': fastest, 'out_pixels': out_px, 'ns_per_out_pixel': ms * 1e6 / out_px,
            'model_MB': nbytes / 1e6, 'model_GBps': nbytes / (ms * 1e-3) / 1e9, 'launches': launches}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--src', default='1024,2048')
    ap.add_argument('--view', default='720,1280')
    ap.add_argument('--hfov', type=float, default=90.0)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    import torch
    from cp_360_weakly_supervised_saliency_amd import ops
    from cp_360_weakly_supervised_saliency_amd.utils import hashrng
    from cp_360_weakly_supervised_saliency_amd.utils import viewport as vp

    assert torch.cuda.is_available(), "viewport_bench needs a GPU"
    F = args.frames
    H, W = (int(v) for v in args.src.split(','))
    h, w = (int(v) for v in args.view.split(','))
    clock = ops.held_clock_ghz() or float('nan')

    def video(n, hh, ww):
        """n u8 frames of hh x ww: eight smooth hash textures of 1 / 8 of the size, enlarged on the device (input preparation)."""
        base = torch.from_numpy(hashrng.uniform(31, (8, 3, max(hh // 8, 2), max(ww // 8, 2)), 0.0, 255.0)).cuda()
        big = torch.nn.functional.interpolate(base, size=(hh, ww), mode='bilinear', align_corners=False)
        big = big.permute(0, 2, 3, 1).round().clamp(0, 255).to(torch.uint8).contiguous()
        return big[torch.arange(n, device='cuda') % 8].contiguous()

    # cameras along a pan that crosses the seam and climbs: 3 degrees a frame
    t = np.deg2rad(150.0 + 3.0 * np.arange(F))
    lat = np.deg2rad(25.0 * np.sin(np.arange(F) / 10.0))
    path = np.stack([np.cos(lat) * np.cos(t), np.sin(lat), np.cos(lat) * np.sin(t)], 1)
    R = torch.from_numpy(vp.cameras(path).astype(np.float32)).cuda()
    rows = []

    frames = video(F, H, W)
    views = torch.empty((F, h, w, 3), dtype=torch.uint8, device='cuda')
    # the source footprint of the views: a border as wide as the view paints every panorama pixel inside it
    zero = torch.zeros_like(frames)
    painted = ops.viewport_outline(zero, R, (h, w), args.hfov, border_px=w, rgb=(1, 1, 1))
    footprint = int(painted[..., 0].sum().item())
    del zero, painted
    ms, fastest = time_ms(lambda: ops.viewport_render(frames, R, (h, w), args.hfov, out=views), args.reps, args.warmup)
    rows.append(row('render u8 %dx%d -> %dx%d' % (H, W, h, w), ms, fastest, F * h * w, 3.0 * (F * h * w + footprint), 1))
    render_ns = rows[-1]['ns_per_out_pixel']

    work = ops._stab_work(0, H, W, frames.device)
    ms, fastest = time_ms(lambda: ops.viewport_outline(frames, R, (h, w), args.hfov, out=frames, work=work), args.reps, args.warmup)
    n_border = int((ops.viewport_outline(torch.zeros_like(frames), R, (h, w), args.hfov, rgb=(1, 1, 1))[..., 0]).sum().item())
    rows.append(row('outline in place %dx%d' % (H, W), ms, fastest, F * H * W, 3.0 * n_border, 2))
    marked = torch.empty_like(frames)
    ms, fastest = time_ms(lambda: ops.viewport_outline(frames, R, (h, w), args.hfov, out=marked, work=work), args.reps, args.warmup)
    rows.append(row('outline copy %dx%d' % (H, W), ms, fastest, F * H * W, 6.0 * F * H * W, 2))
    del marked

    flat = video(F, h, w)
    flat_out = torch.empty_like(flat)
    small = torch.from_numpy(np.stack([np.eye(3, dtype=np.float32)] * F)).cuda()
    small[:] = R                                                       # the same rotations, read as K11's
    fwork = ops._stab_work(0, h, w, flat.device)
    ms, fastest = time_ms(lambda: ops.equirect_rotate(flat, small, out=flat_out, work=fwork), args.reps, args.warmup)
    rows.append(row('stab_rotate u8 %dx%d (yardstick)' % (h, w), ms, fastest, F * h * w, 6.0 * F * h * w, 2))
    rotate_ns = rows[-1]['ns_per_out_pixel']
    # ... and again after it, alternating, to see the spread of the pair
    ms2, _ = time_ms(lambda: ops.viewport_render(frames, R, (h, w), args.hfov, out=views), args.reps, args.warmup)
    ms3, _ = time_ms(lambda: ops.equirect_rotate(flat, small, out=flat_out, work=fwork), args.reps, args.warmup)
    del flat, flat_out

    pilot = vp.ViewportPilot((h, w), args.hfov)
    planner = vp.ViewportPilot((h, w), args.hfov, planner='viterbi')
    follow, paths = {}, {}
    for hm, wm in ((14, 28), (32, 64)):
        maps = torch.from_numpy(hashrng.uniform(32, (F, hm, wm), 0.0, 0.1)).cuda()
        for f in range(F):
            y, x = int((0.5 - lat[f] / np.pi) * hm) % hm, int((t[f] / (2 * np.pi) + 0.5) * wm) % wm
            maps[f, y, x] += 1.0
        mwork = ops._stab_work(0, hm, wm, maps.device)
        ms, fastest = time_ms(lambda: ops.sphere_smooth(maps, 15.0, work=mwork), args.reps, args.warmup)
        rows.append(row('smooth %dx%d' % (hm, wm), ms, fastest, F * hm * wm, 8.0 * F * hm * wm, 2))
        sm = ops.sphere_smooth(maps, 15.0, work=mwork)
        ms, fastest = time_ms(lambda: ops.sphere_peak(maps, 15.0, smooth=sm, work=mwork), args.reps, args.warmup)
        rows.append(row('peak %dx%d' % (hm, wm), ms, fastest, F * hm * wm, 8.0 * F * hm * wm, 2))
        val = ops.sphere_peak(maps, 15.0, smooth=sm, work=mwork)[2]
        for S in (1, 64):
            sm_s, gain_s, maps_s = sm.repeat(S, 1, 1), (4096.0 / val).repeat(S), maps.repeat(S, 1, 1)
            starts = torch.arange(0, S * F + 1, F, dtype=torch.int32, device='cuda')
            pwork = ops._work(ops.lib().cp360_path_work_bytes, 'sphere_path', S * F, hm, wm, maps.device, None)
            ms, fastest = time_ms(lambda: ops.sphere_path(sm_s, gain_s, starts=starts, work=pwork), args.reps, args.warmup)
            rows.append(row('path %dx%d, %d x %d frames' % (hm, wm, S, F), ms, fastest, S * F * hm * wm, 6.0 * S * F * hm * wm, 3))
            idx = ops.sphere_path(sm_s, gain_s, starts=starts, work=pwork)[0]
            ms, fastest = time_ms(lambda: ops.sphere_refine(maps_s, idx, 15.0, work=mwork), args.reps, args.warmup)
            rows.append(row('refine %dx%d, %d x %d frames' % (hm, wm, S, F), ms, fastest, S * F * hm * wm, 4.0 * S * F * hm * wm, 2))
            del sm_s, gain_s, maps_s, pwork
        ms, _ = time_ms(lambda: pilot.follow(frames, maps), args.reps, args.warmup)
        follow['%dx%d' % (hm, wm)] = {'ms_per_call': ms, 'ms_per_frame': ms / F}
        ms_peak, _ = time_ms(lambda: pilot.path(maps), args.reps, args.warmup)
        ms_plan, _ = time_ms(lambda: planner.path(maps), args.reps, args.warmup)
        paths['%dx%d' % (hm, wm)] = {'peak_ms_per_call': ms_peak, 'viterbi_ms_per_call': ms_plan}

    print('%d frames; held shader clock under a bare MFMA loop %.3f GHz; median of %d after %d warm-up calls (HIP events)'
          % (F, clock, args.reps, args.warmup))
    print('%-40s %10s %12s %14s %10s %10s' % ('kernel', 'ms / call', 'min ms', 'ns / out pixel', 'model MB', 'GB/s'))
    for r in rows:
        print('%-40s %10.3f %12.3f %14.4f %10.2f %10.1f' % (r['kernel'], r['ms_per_call'], r['min_ms_per_call'], r['ns_per_out_pixel'],
                                                           r['model_MB'], r['model_GBps']))
    print('render / stab_rotate per output pixel: %.2f (again, after the others: %.3f / %.3f ms = %.2f); source footprint %.1f %% of '
          'the panorama per view' % (render_ns / rotate_ns, ms2, ms3, ms2 / ms3, 100.0 * footprint / (F * H * W)))
    for k, v in follow.items():
        print('follow, maps %s: %.3f ms / call, %.3f ms / frame' % (k, v['ms_per_call'], v['ms_per_frame']))
    for k, v in paths.items():
        print(".path, maps %s: planner 'peak' %.3f ms / call, 'viterbi' %.3f ms / call" % (k, v['peak_ms_per_call'], v['viterbi_ms_per_call']))
    print(json.dumps({'tool': 'viewport_bench', 'frames': F, 'src': [H, W], 'view': [h, w], 'hfov_deg': args.hfov,
                      'held_clock_ghz': clock, 'rows': rows, 'render_over_rotate': render_ns / rotate_ns,
                      'render_over_rotate_again': ms2 / ms3, 'footprint_fraction': footprint / (F * H * W), 'follow': follow, 'path': paths}))


if __name__ == '__main__':
    main()
