#!/usr/bin/env python
"""Times the streaming kernels (K24, csrc/streaming.hip) on one video: F frames of 14 x 28 saliency maps, the grid 120 x 240 in
6 x 12 tiles, a square window of 100 degrees, V viewers per frame and a ladder of three levels.

  incidence   ops.view_incidence: the tables and one launch, S P (camera, pixel) tests - once per planner, not per video
  tiles       ops.tile_incidence: one launch over the S rows of bits
  expect      ops.view_expect on the pixels (P outputs a frame) and on the tiles (T outputs a frame): F P S conditional additions
              in the definition's order, one division per output; it reads 4 F S bytes of maps and S P / 8 bytes of bits per four
              frames (from the caches after the first workgroups) and writes 4 F P bytes
  quality     ops.view_quality: the tables and one launch, N P tests (N = F V pairs)
  torch       the expectation composed from torch: the masses [F, S] times the incidence as a float32 [S, P] matrix, a library
              GEMM of 2 F P S operations, and the division by the row totals.  A fair competitor: it may win on time.  Its sums
              are in the library's order, not the definition's, and it keeps S P floats where the kernel keeps S P bits.

HIP events around each call, the median after warm-up, workspace reused; the clock is the one the chip holds under a matrix
load right after the timed calls (ops.held_clock_ghz), noted beside the times.
  python tools/streaming_bench.py [--frames 1800] [--viewers 48] [--reps 20] [--warmup 5] [--out profiles/streaming_bench.md]
Prints a table and one JSON line; --out writes both as markdown."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.headtrack_bench import time_ms, viewers                     # noqa: E402  the same viewers, the same timer


def maps(F, target, hw):
    """A blob of 12 degrees on the target and a weaker, fixed one, on a floor: float32 [F, hs, ws], every value positive."""
    hs, ws = hw
    phi = ((1.0 - 2.0 * (np.arange(hs) + 0.5) / hs) * np.pi / 2.0)[:, None]
    theta = ((2.0 * (np.arange(ws) + 0.5) / ws - 1.0) * np.pi)[None, :]
    p = np.stack([np.cos(phi) * np.cos(theta), np.sin(phi) * np.ones_like(theta), np.cos(phi) * np.sin(theta)], -1)
    kappa = 1.0 / np.deg2rad(12.0) ** 2
    fixed = np.array([-0.5, 0.1, 0.86])
    fixed /= np.linalg.norm(fixed)
    blob = np.exp(kappa * (np.einsum('yxc,fc->fyx', p, target) - 1.0)) + 0.4 * np.exp(kappa * (p @ fixed - 1.0))[None]
    return (blob + 1e-3).astype(np.float32)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--frames', type=int, default=1800)
    ap.add_argument('--viewers', type=int, default=48)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from cp_360_weakly_supervised_saliency_amd import ops
    from cp_360_weakly_supervised_saliency_amd.utils import streaming

    assert torch.cuda.is_available(), "streaming_bench needs a GPU"
    F, V, (hs, ws), (h, w), tiles, view, L = args.frames, args.viewers, (14, 28), (120, 240), (6, 12), ((1, 1), 100.0), 3
    S, P, T = hs * ws, h * w, tiles[0] * tiles[1]
    R_np, offsets_np, target = viewers(F, V)
    R, offsets = torch.from_numpy(R_np).cuda(), torch.from_numpy(offsets_np).cuda()
    N = int(R.shape[0])
    sal = torch.from_numpy(maps(F, target, (hs, ws))).cuda()
    dev = sal.device
    cams = torch.from_numpy(streaming.gaze_cameras((hs, ws))).cuda()
    a_src, a = ops.sphere_eval_weights(hs, 'solid_angle', dev), ops.sphere_eval_weights(h, 'solid_angle', dev)
    work = ops.view_quality_work(h, w, dev)
    inc = ops.view_incidence(cams, (h, w), view[0], view[1], work=work)
    tinc = ops.tile_incidence(inc, (h, w), tiles)
    out, total = ops.view_expect(sal, a_src, inc, P)
    levels = (torch.arange(F * T, device=dev).view(F, T) % L).to(torch.uint8)
    out_buf, vis_buf = torch.empty((F, P), device=dev), torch.empty((F, T), device=dev)

    # the torch composition, checked against the kernel before it is timed
    shifts = torch.arange(32, device=dev, dtype=torch.int32)
    dense = ((inc[:, :, None] >> shifts) & 1).reshape(S, -1)[:, :P].to(torch.float32).contiguous()        # [S, P]
    a_px = a_src.to(torch.float32).repeat_interleave(ws)

    def torch_expect():
        flat = sal.view(F, S)
        m = torch.where((flat > 0) & torch.isfinite(flat), flat * a_px, torch.zeros_like(flat))
        tot = m.sum(dim=1, keepdim=True)
        return torch.matmul(m, dense) / tot

    differ = float((torch_expect() - out).abs().max())

    ms = {}
    ms['incidence'] = time_ms(lambda: ops.view_incidence(cams, (h, w), view[0], view[1], work=work, out=inc), args.reps, args.warmup)
    ms['tiles'] = time_ms(lambda: ops.tile_incidence(inc, (h, w), tiles, out=tinc), args.reps, args.warmup)
    ms['expect_pixels'] = time_ms(lambda: ops.view_expect(sal, a_src, inc, P, out=out_buf), args.reps, args.warmup)
    ms['expect_tiles'] = time_ms(lambda: ops.view_expect(sal, a_src, tinc, T, out=vis_buf), args.reps, args.warmup)
    ms['quality'] = time_ms(lambda: ops.view_quality(R, offsets, (h, w), view, a, levels, tiles, L, work=work), args.reps, args.warmup)
    ms['torch_expect'] = time_ms(torch_expect, args.reps, args.warmup)
    ghz = ops.held_clock_ghz()
    cus = torch.cuda.get_device_properties(0).multi_processor_count

    sp = streaming.StreamPlanner((h, w), (hs, ws), view[0], view[1], tiles)
    rates = [1.0e6, 4.0e6, 1.6e7]
    plan = sp.evaluate(sal, R, offsets, rates, rates[1] * (1.0 + 1e-9), 30.0)

    adds = float(F) * P * S
    res = {'tool': 'streaming_bench', 'frames': F, 'viewers': V, 'pairs': N, 'src': [hs, ws], 'grid': [h, w], 'tiles': list(tiles),
           'view': view, 'levels': L, 'reps': args.reps, 'warmup': args.warmup, 'held_clock_ghz': ghz, 'cus': cus,
           'inc_bytes': inc.numel() * 4, 'dense_bytes': dense.numel() * 4, 'work_KB': work.numel() * 8 / 1e3,
           'expect_adds': adds, 'gemm_flops': 2.0 * adds, 'torch_max_abs_diff': differ,
           'plan_utility': plan['plan_utility'], 'uniform_utility': plan['uniform_utility'], 'plan_bits': plan['plan_bits'],
           'uniform_bits': plan['uniform_bits']}
    for k, (med, mn) in ms.items():
        res[k + '_ms'], res[k + '_min_ms'] = med, mn
    res['expect_pixels_adds_per_s'] = adds / (res['expect_pixels_ms'] * 1e-3)
    res['torch_expect_flops_per_s'] = 2.0 * adds / (res['torch_expect_ms'] * 1e-3)
    res['quality_tests_per_s'] = float(N) * P / (res['quality_ms'] * 1e-3)
    res['incidence_tests_per_s'] = float(S) * P / (res['incidence_ms'] * 1e-3)
    lines = ['F = %d frames of %d x %d maps (S = %d), grid %d x %d (P = %d), %d x %d tiles (T = %d), window %s, %d viewers a frame = %d pairs, %d levels'
             % (F, hs, ws, S, h, w, P, tiles[0], tiles[1], T, view, V, N, L),
             'median of %d after %d warm-up calls (HIP events); held clock %.2f GHz, %d CUs' % (args.reps, args.warmup, ghz, cus),
             'incidence (K24a)         %9.3f ms / call   (min %.3f)   %.3e tests / s; once per planner' % (res['incidence_ms'], res['incidence_min_ms'], res['incidence_tests_per_s']),
             'tile incidence (K24b)    %9.3f ms / call   (min %.3f)' % (res['tiles_ms'], res['tiles_min_ms']),
             'expect, pixels (K24c)    %9.3f ms / call   (min %.3f)   %.3e conditional additions / s' % (res['expect_pixels_ms'], res['expect_pixels_min_ms'], res['expect_pixels_adds_per_s']),
             'expect, tiles (K24c)     %9.3f ms / call   (min %.3f)' % (res['expect_tiles_ms'], res['expect_tiles_min_ms']),
             'quality (K24d)           %9.3f ms / call   (min %.3f)   %.3e tests / s' % (res['quality_ms'], res['quality_min_ms'], res['quality_tests_per_s']),
             'torch expect, pixels     %9.3f ms / call   (min %.3f)   %.3e FLOP / s; max |torch - K24c| = %.3e'
             % (res['torch_expect_ms'], res['torch_expect_min_ms'], res['torch_expect_flops_per_s'], differ),
             'incidence memory         %9.1f KB as bits, %.1f KB as the float32 matrix of the torch composition' % (res['inc_bytes'] / 1e3, res['dense_bytes'] / 1e3),
             'workspace                %9.1f KB' % res['work_KB'],
             'plan at the budget of uniform level 1: utility %.4f (%.0f bits a segment) against %.4f (%.0f bits) of the uniform plan'
             % (res['plan_utility'], res['plan_bits'], res['uniform_utility'], res['uniform_bits'])]
    print('\n'.join(lines))
    print(json.dumps(res))
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write('# tools/streaming_bench.py on one MI355X\n\n```\n' + '\n'.join(lines) + '\n```\n\nThe JSON line of the run:\n\n```\n'
                     + json.dumps(res) + '\n```\n')


if __name__ == '__main__':
    main()
