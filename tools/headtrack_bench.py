#!/usr/bin/env python
"""Times the head-tracking kernels (K17, csrc/headtrack.hip) on one video per call: F frames of 120 x 240, V viewers per frame with
a square window of 100 degrees, judged against a camera of 36 x 64 / 90 degrees.

  footprints  ops.head_footprints: the tables and one launch; F V P (camera, pixel) tests
  agreement   ops.head_agreement: the tables and one launch; 2 F V P tests (the camera's and the viewer's window per pixel)
  torch       the same definitions composed from torch on the GPU: a batched matmul of the pixel directions with the cameras, the
              two quotients, the compares and the (weighted) sums.  It materialises [N, P, 3] floats and [N, P] booleans, so it is
              timed on --torch-frames frames of the video and set against the kernels by its rate

A test is 9 multiplications, 6 additions, 2 divisions and 3 comparisons of float32: 20 operations where a division counts as one.
The operation bound is 20 lane-operations a test at the rate the chip issues float32 vector instructions, 128 lanes a clock and CU
at the held clock (an IEEE division is not one instruction: the fraction says how far the kernels are from a loop of nothing but
the definition's terms at one instruction each).  Pairs are (frame, viewer) pairs.

HIP events around each call, the median after warm-up, workspace reused.
  python tools/headtrack_bench.py [--frames 1800] [--viewers 48] [--torch-frames 30] [--reps 20] [--warmup 5] [--out profiles/headtrack_bench.md]
Prints a table and one JSON line; --out writes both as markdown."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

OPS_PER_TEST = 20.0


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


def viewers(F, V, fps=30.0):
    """A target that drifts in longitude and sways in latitude; V viewers follow it with fixed offsets (normal, 8 degrees), a
    slow roll and tracks sampled at 10 Hz -> head_cameras' (R, offsets) and the target's directions [F, 3]."""
    from cp_360_weakly_supervised_saliency_amd.utils import hashrng, headtrack
    t = np.arange(int(F / fps * 10.0) + 2) * 0.1
    lon = np.deg2rad(20.0) * t
    lat = np.deg2rad(25.0) * np.sin(0.7 * t)
    d = np.deg2rad(8.0) * hashrng.normal(51, (V, 2), dtype=np.float64)
    tracks = [(t, lon + d[v, 0], np.clip(lat + d[v, 1], -1.5, 1.5), np.deg2rad(5.0) * np.sin(0.3 * t + v)) for v in range(V)]
    R, offsets, _ = headtrack.head_cameras(tracks, fps, F)
    tf = (np.arange(F) + 0.5) / fps
    lo, la = np.deg2rad(20.0) * tf, np.deg2rad(25.0) * np.sin(0.7 * tf)
    return R, offsets, np.stack([np.cos(la) * np.cos(lo), np.sin(la), np.cos(la) * np.sin(lo)], -1)


def pixel_dirs(h, w):
    """The directions of the grid's pixel centres, float32 [h w, 3]: the tables' (cos, sin) rounded once, then multiplied."""
    theta = np.pi * ((2.0 * np.arange(w) + 1.0) / w - 1.0)
    phi = np.pi * 0.5 * (1.0 - (2.0 * np.arange(h) + 1.0) / h)
    ct, st, cp, sp = (v.astype(np.float32) for v in (np.cos(theta), np.sin(theta), np.cos(phi), np.sin(phi)))
    return np.stack([cp[:, None] * ct[None, :], np.broadcast_to(sp[:, None], (h, w)), cp[:, None] * st[None, :]], -1).reshape(-1, 3)


def tangents(view):
    """(tx, ty) of a view ((h_v, w_v), hfov_deg) as the library rounds them to float32."""
    t = np.tan(0.5 * np.deg2rad(view[1]))
    return float(np.float32(t)), float(np.float32(t * (view[0][0] / view[0][1])))


def torch_inside(R, dirs, tx, ty):
    """R [N, 3, 3], dirs [P, 3] -> bool [N, P]: the definition, composed from torch."""
    import torch
    d = torch.matmul(dirs[None], R)                                    # p^T R = (d_f, d_u, d_r)
    df = d[:, :, 0]
    ok = torch.isfinite(R).all(dim=2).all(dim=1)[:, None]
    return (df > 0) & ((d[:, :, 2] / df).abs() <= tx) & ((d[:, :, 1] / df).abs() <= ty) & ok


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--frames', type=int, default=1800)
    ap.add_argument('--viewers', type=int, default=48)
    ap.add_argument('--torch-frames', type=int, default=30)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from cp_360_weakly_supervised_saliency_amd import ops
    from cp_360_weakly_supervised_saliency_amd.utils import headtrack, viewport

    assert torch.cuda.is_available(), "headtrack_bench needs a GPU"
    F, V, h, w = args.frames, args.viewers, 120, 240
    P = h * w
    view, cam_view = ((1, 1), 100.0), ((36, 64), 90.0)
    R_np, offsets_np, target = viewers(F, V)
    R, offsets = torch.from_numpy(R_np).cuda(), torch.from_numpy(offsets_np).cuda()
    N = int(R.shape[0])
    assert N == F * V
    Rc = torch.from_numpy(viewport.cameras(target).astype(np.float32)).cuda()
    a = ops.sphere_eval_weights(h, 'solid_angle', R.device)
    work = ops.head_work(h, w, R.device)
    head = headtrack.HeadMaps((h, w), view[0], view[1])
    means = head.means(head.agreement(Rc, cam_view[0], cam_view[1], R, offsets))
    counts, n_views = ops.head_footprints(R, offsets, (h, w), view[0], view[1], work=work)
    inter, uni = ops.head_agreement(Rc, cam_view, R, offsets, (h, w), view, a, work=work)
    assert n_views.tolist() == [V] * F

    # the torch composition on the first frames of the video, checked against the kernels before it is timed
    Ft = min(args.torch_frames, F)
    Nt = Ft * V
    dirs = torch.from_numpy(pixel_dirs(h, w)).cuda()
    (tx, ty), (ctx, cty) = tangents(view), tangents(cam_view)
    frame = torch.arange(Nt, device=R.device) // V
    a_px = a.to(torch.int64).repeat_interleave(w)

    def torch_footprints():
        return torch_inside(R[:Nt], dirs, tx, ty).view(Ft, V, P).sum(dim=1, dtype=torch.int32)

    def torch_agreement():
        v, c = torch_inside(R[:Nt], dirs, tx, ty), torch_inside(Rc[:Ft], dirs, ctx, cty)[frame]
        return ((v & c) * a_px).sum(dim=1), ((v | c) * a_px).sum(dim=1)

    differ = int((torch_footprints() != counts[:Ft].view(Ft, P)).sum())    # torch's matmul may contract: a few knife edges
    ti, tu = torch_agreement()
    differ_pairs = int(((ti != inter[:Nt]) | (tu != uni[:Nt])).sum())

    ms_f, min_f = time_ms(lambda: ops.head_footprints(R, offsets, (h, w), view[0], view[1], work=work), args.reps, args.warmup)
    ms_a, min_a = time_ms(lambda: ops.head_agreement(Rc, cam_view, R, offsets, (h, w), view, a, work=work), args.reps, args.warmup)
    ms_tf, _ = time_ms(torch_footprints, args.reps, args.warmup)
    ms_ta, _ = time_ms(torch_agreement, args.reps, args.warmup)
    ghz = ops.held_clock_ghz()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    lane_rate = 128.0 * cus * ghz * 1e9
    tests_f, tests_a = float(N) * P, 2.0 * N * P
    bound_f, bound_a = tests_f * OPS_PER_TEST / lane_rate * 1e3, tests_a * OPS_PER_TEST / lane_rate * 1e3
    res = {'tool': 'headtrack_bench', 'frames': F, 'viewers': V, 'grid': [h, w], 'view': view, 'cam_view': cam_view, 'pairs': N,
           'reps': args.reps, 'warmup': args.warmup, 'mean_frame_iou': means['iou'], 'mean_centre_angle_deg': means['centre_angle_deg'],
           'footprints_ms': ms_f, 'footprints_min_ms': min_f, 'footprints_pairs_per_s': N / (ms_f * 1e-3),
           'footprints_tests_per_s': tests_f / (ms_f * 1e-3), 'footprints_bound_ms': bound_f, 'footprints_of_bound': bound_f / ms_f,
           'agreement_ms': ms_a, 'agreement_min_ms': min_a, 'agreement_pairs_per_s': N / (ms_a * 1e-3),
           'agreement_tests_per_s': tests_a / (ms_a * 1e-3), 'agreement_bound_ms': bound_a, 'agreement_of_bound': bound_a / ms_a,
           'torch_frames': Ft, 'torch_pairs': Nt, 'torch_footprints_ms': ms_tf, 'torch_footprints_pairs_per_s': Nt / (ms_tf * 1e-3),
           'torch_agreement_ms': ms_ta, 'torch_agreement_pairs_per_s': Nt / (ms_ta * 1e-3),
           'torch_pixels_that_differ': differ, 'torch_pairs_that_differ': differ_pairs,
           'ops_per_test': OPS_PER_TEST, 'held_clock_ghz': ghz, 'cus': cus, 'lane_ops_per_s': lane_rate,
           'work_KB': work.numel() * 8 / 1e3}
    lines = ['F = %d frames of %d x %d, %d viewers per frame = %d pairs; windows %s (viewers) and %s (camera)' % (F, h, w, V, N, view, cam_view),
             'mean frame IoU %.4f, mean centre angle %.2f degrees' % (means['iou'], means['centre_angle_deg']),
             'median of %d after %d warm-up calls (HIP events); held clock %.2f GHz, %d CUs, %.3e f32 lane-operations / s'
             % (args.reps, args.warmup, ghz, cus, lane_rate),
             'footprints (K17a)        %9.3f ms / call   %.3e pairs / s, %.3e tests / s; bound %.3f ms = %.3f of the time'
             % (ms_f, res['footprints_pairs_per_s'], res['footprints_tests_per_s'], bound_f, res['footprints_of_bound']),
             'agreement (K17b)         %9.3f ms / call   %.3e pairs / s, %.3e tests / s; bound %.3f ms = %.3f of the time'
             % (ms_a, res['agreement_pairs_per_s'], res['agreement_tests_per_s'], bound_a, res['agreement_of_bound']),
             'torch footprints         %9.3f ms / %d frames   %.3e pairs / s   (%d of %d counts differ from K17a)'
             % (ms_tf, Ft, res['torch_footprints_pairs_per_s'], differ, Ft * P),
             'torch agreement          %9.3f ms / %d frames   %.3e pairs / s   (%d of %d pairs differ from K17b)'
             % (ms_ta, Ft, res['torch_agreement_pairs_per_s'], differ_pairs, Nt),
             'workspace                %9.1f KB' % res['work_KB']]
    print('\n'.join(lines))
    print(json.dumps(res))
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write('# tools/headtrack_bench.py on one MI355X\n\n```\n' + '\n'.join(lines) + '\n```\n\nThe JSON line of the run:\n\n```\n'
                     + json.dumps(res) + '\n```\n')


if __name__ == '__main__':
    main()
