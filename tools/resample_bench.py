#!/usr/bin/env python
"""Times the conservative remap on the sphere (K25, csrc/sphere_resample.hip), forward and adjoint, on F fine maps:

  forward    ops.sphere_resample: one launch that reads every source pixel once (4 F hs ws bytes) and writes 4 F h w bytes
  adjoint    ops.sphere_resample_adjoint: one launch that writes every source pixel once
  torch      the same remap composed from torch on the same device, Wy @ src @ Wx^T with dense float32 matrices
             (temporal_model.train_supervised.resample_conservative_torch), and its transpose Wy^T @ g @ Wx.  A fair competitor:
             a library GEMM may win on time.  Its sums are in the library's order, and it keeps the [h, hs] and [w, ws] matrices
  copy       a plain device copy of the source bytes in the same run: the floor of a kernel that must read every source pixel
             (a copy reads and writes them: its bytes / s, not its time, is the yardstick; the floor is half its time)
  bilinear   ops.sphere_eval_resample on the same shapes: four taps per grid pixel, not the same work - what the opt-in costs

HIP events around each call, the median after warm-up; the clock is the one the chip holds under a matrix load right after the
timed calls (ops.held_clock_ghz), noted beside the times.
  python tools/resample_bench.py [--frames 64] [--reps 20] [--warmup 5] [--out profiles/resample_bench.md]
Prints a table and one JSON line; --out writes both as markdown."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.headtrack_bench import time_ms                              # noqa: E402  the same timer

SHAPES = [((1024, 2048), (120, 240)), ((1024, 2048), (30, 60)), ((2048, 4096), (120, 240))]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from cp_360_weakly_supervised_saliency_amd import ops
    from cp_360_weakly_supervised_saliency_amd.temporal_model import train_supervised as ts

    assert torch.cuda.is_available(), "resample_bench needs a GPU"
    F = args.frames
    rows, lines = [], []
    for (hs, ws), (h, w) in SHAPES:
        gen = torch.Generator(device='cuda').manual_seed(25)
        src = torch.rand((F, hs, ws), generator=gen, device='cuda', dtype=torch.float32)
        g = torch.rand((F, h, w), generator=gen, device='cuda', dtype=torch.float32)
        plan = ops.sphere_resample_plan((hs, ws), (h, w), src.device)
        out, dup = torch.empty((F, h, w), device=src.device), torch.empty_like(src)
        Wy = torch.from_numpy(ts._conservative_matrix(hs, h, 0)).cuda()
        Wx = torch.from_numpy(ts._conservative_matrix(ws, w, 1)).cuda()
        WxT, WyT = Wx.t().contiguous(), Wy.t().contiguous()
        torch_fwd = lambda: torch.matmul(torch.matmul(Wy, src), WxT)
        torch_adj = lambda: torch.matmul(torch.matmul(WyT, g), Wx)
        # the torch composition against the kernels before either is timed
        d_fwd = float((torch_fwd() - ops.sphere_resample(src, (h, w), plan=plan)).abs().max())
        adj = ops.sphere_resample_adjoint(g, (hs, ws), plan=plan)
        d_adj = float((torch_adj() - adj).abs().max() / adj.abs().max())
        ms = {}
        ms['forward'] = time_ms(lambda: ops.sphere_resample(src, (h, w), plan=plan, out=out), args.reps, args.warmup)
        ms['adjoint'] = time_ms(lambda: ops.sphere_resample_adjoint(g, (hs, ws), plan=plan), args.reps, args.warmup)
        ms['torch_forward'] = time_ms(torch_fwd, args.reps, args.warmup)
        ms['torch_adjoint'] = time_ms(torch_adj, args.reps, args.warmup)
        ms['copy'] = time_ms(lambda: dup.copy_(src), args.reps, args.warmup)
        ms['bilinear'] = time_ms(lambda: ops.sphere_eval_resample(src, (h, w), out=out), args.reps, args.warmup)
        src_bytes = 4.0 * F * hs * ws
        row = {'src': [hs, ws], 'grid': [h, w], 'src_MB': src_bytes / 1e6, 'run_cap': [int(ops.lib().cp360_sresample_run_cap(hs, h)),
                                                                                      int(ops.lib().cp360_sresample_run_cap(ws, w))],
               'plan_bytes': int(plan.numel()), 'dense_bytes': int(Wy.numel() + Wx.numel()) * 4,
               'torch_forward_max_abs_diff': d_fwd, 'torch_adjoint_max_rel_diff': d_adj}
        for k, (med, mn) in ms.items():
            row[k + '_ms'], row[k + '_min_ms'] = med, mn
        row['forward_GBps'] = src_bytes / (row['forward_ms'] * 1e-3) / 1e9
        row['adjoint_GBps'] = src_bytes / (row['adjoint_ms'] * 1e-3) / 1e9
        row['copy_GBps'] = 2.0 * src_bytes / (row['copy_ms'] * 1e-3) / 1e9
        row['read_floor_ms'] = 0.5 * row['copy_ms']
        rows.append(row)
        lines += ['%d x %d -> %d x %d, F = %d (%.0f MB of source; runs of up to %d rows x %d columns; plan %.1f KB, dense matrices %.1f KB)'
                  % (hs, ws, h, w, F, row['src_MB'], row['run_cap'][0], row['run_cap'][1], row['plan_bytes'] / 1e3, row['dense_bytes'] / 1e3),
                  '  forward (K25)          %9.3f ms / call   (min %.3f)   %7.1f GB / s of source read' % (row['forward_ms'], row['forward_min_ms'], row['forward_GBps']),
                  '  adjoint (K25)          %9.3f ms / call   (min %.3f)   %7.1f GB / s of source written' % (row['adjoint_ms'], row['adjoint_min_ms'], row['adjoint_GBps']),
                  '  torch forward          %9.3f ms / call   (min %.3f)   max |torch - K25| = %.3e' % (row['torch_forward_ms'], row['torch_forward_min_ms'], d_fwd),
                  '  torch adjoint          %9.3f ms / call   (min %.3f)   max |torch - K25| / max = %.3e' % (row['torch_adjoint_ms'], row['torch_adjoint_min_ms'], d_adj),
                  '  device copy of source  %9.3f ms / call   (min %.3f)   %7.1f GB / s read + written; reading alone: %.3f ms'
                  % (row['copy_ms'], row['copy_min_ms'], row['copy_GBps'], row['read_floor_ms']),
                  '  bilinear (K14)         %9.3f ms / call   (min %.3f)   four taps per grid pixel: not the same work' % (row['bilinear_ms'], row['bilinear_min_ms'])]
        del src, dup, g, out, adj
        torch.cuda.empty_cache()
    ghz = ops.held_clock_ghz()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    head = ['median of %d after %d warm-up calls (HIP events); held clock %.2f GHz, %d CUs' % (args.reps, args.warmup, ghz, cus)]
    res = {'tool': 'resample_bench', 'frames': F, 'reps': args.reps, 'warmup': args.warmup, 'held_clock_ghz': ghz, 'cus': cus, 'shapes': rows}
    print('\n'.join(head + lines))
    print(json.dumps(res))
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write('# tools/resample_bench.py on one MI355X\n\n```\n' + '\n'.join(head + lines) + '\n```\n\nThe JSON line of the run:\n\n```\n'
                     + json.dumps(res) + '\n```\n')


if __name__ == '__main__':
    main()
