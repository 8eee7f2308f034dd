#!/usr/bin/env python
"""Times the video quality measurement on the sphere (K26, csrc/sphere_quality.hip) on F frame pairs of 1024 x 2048 and of
2048 x 4096, on cells 6 x 12 and 120 x 240, the squared error alone and with the structural similarity:

  K26        ops.sphere_quality: one pass that reads both videos once (2 x 3 F H W bytes)
  copy       a plain device copy of one video in the same run: it reads and writes 3 F H W bytes each, so its bytes / s is the
             yardstick and its time is the floor of a kernel that must read two videos (the same number of bytes moved)
  torch      the same definition composed from torch on the device: int64 squared differences and ``index_add_`` into the cells,
             reshaped sums for the blocks, ``roll`` for the windows, float64 for the quotient; in chunks of 8 frames (its int64
             temporaries are 8 times the frames).  Checked equal to the kernel before either is timed.

HIP events around each call, the median after warm-up; the clock is the one the chip holds under a matrix load right after the
timed calls (ops.held_clock_ghz), noted beside the times.
  python tools/quality_bench.py [--frames 64] [--reps 20] [--warmup 5] [--torch-reps 3] [--out profiles/quality_bench.md]
Prints a table and one JSON line; --out writes both as markdown."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.headtrack_bench import time_ms                              # noqa: E402  the same timer

SIZES = [(1024, 2048), (2048, 4096)]
CELLS = [(6, 12), (120, 240)]


def torch_quality(ref, dist, cells, a, ssim, chunk=8):
    """The definition of DESIGN 7r in torch, on ref's device -> (sse, ssim_q or None)."""
    import torch
    F, H, W, _ = ref.shape
    rows, cols = cells
    dev = ref.device
    cy = (torch.arange(H, device=dev) * rows) // H
    cx = (torch.arange(W, device=dev) * cols) // W
    t = (cy[:, None] * cols + cx[None, :]).reshape(-1)
    a = a.to(torch.int64)
    sse = torch.zeros((F, rows * cols, 3), dtype=torch.int64, device=dev)
    q_out = torch.zeros((F, rows * cols), dtype=torch.int64, device=dev) if ssim else None
    if ssim:
        i, j = torch.arange(H // 4 - 1, device=dev), torch.arange(W // 4, device=dev)
        ww = torch.stack([a[4 * i + r] for r in range(8)]).sum(dim=0)
        wt = (cy[4 * i + 4][:, None] * cols + cx[(4 * j + 4) % W][None, :]).reshape(-1)
    for f0 in range(0, F, chunk):
        r, d = ref[f0:f0 + chunk].to(torch.int64), dist[f0:f0 + chunk].to(torch.int64)
        n = r.shape[0]
        e = (r - d) ** 2 * a[None, :, None, None]
        sse[f0:f0 + n].index_add_(1, t, e.reshape(n, H * W, 3))
        if ssim:
            yr = (4899 * r[..., 0] + 9617 * r[..., 1] + 1868 * r[..., 2] + 8192) >> 14
            yd = (4899 * d[..., 0] + 9617 * d[..., 1] + 1868 * d[..., 2] + 8192) >> 14

            def win(v):
                b = v.reshape(n, H // 4, 4, W // 4, 4).sum(dim=(2, 4))
                b = b + torch.roll(b, -1, dims=2)
                return b[:, :-1] + b[:, 1:]

            s1, s2, ss, s12 = win(yr), win(yd), win(yr * yr + yd * yd), win(yr * yd)
            A = (2 * s1 * s2 + 416) * (2 * (64 * s12 - s1 * s2) + 235963)
            B = (s1 * s1 + s2 * s2 + 416) * (64 * ss - s1 * s1 - s2 * s2 + 235963)
            q = torch.round(A.to(torch.float64) / B.to(torch.float64) * 16777216.0).to(torch.int64)
            q_out[f0:f0 + n].index_add_(1, wt, (q * ww[None, :, None]).reshape(n, -1))
    return sse, q_out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--torch-reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from cp_360_weakly_supervised_saliency_amd import ops

    assert torch.cuda.is_available(), "quality_bench needs a GPU"
    F = args.frames
    rows, lines = [], []
    for H, W in SIZES:
        gen = torch.Generator(device='cuda').manual_seed(26)
        ref = torch.randint(0, 256, (F, H, W, 3), generator=gen, device='cuda', dtype=torch.uint8)
        dist = (ref.to(torch.int16) + torch.randint(-6, 7, ref.shape, generator=gen, device='cuda', dtype=torch.int16)).clamp_(0, 255).to(torch.uint8)
        dup = torch.empty_like(ref)
        a = ops.shot_weights(H, ref.device)
        video = 3.0 * F * H * W
        copy_ms, copy_min = time_ms(lambda: dup.copy_(ref), args.reps, args.warmup)
        copy_gbps = 2.0 * video / (copy_ms * 1e-3) / 1e9
        lines.append('%d x %d, F = %d (two videos of %.0f MB): device copy of one video %.3f ms (min %.3f), %.1f GB / s read + written - '
                     'the floor of reading both' % (H, W, F, video / 1e6, copy_ms, copy_min, copy_gbps))
        del dup
        for cells in CELLS:
            work = ops.sphere_quality_work(F, H, W, cells, ref.device)
            for ssim in (False, True):
                got = ops.sphere_quality(ref, dist, cells, ssim=ssim, work=work)
                want = torch_quality(ref, dist, cells, a, ssim)
                equal = bool(torch.equal(got[0], want[0]) and (not ssim or torch.equal(got[1], want[1])))
                assert equal, "the torch composition and K26 differ on %d x %d, cells %r, ssim %r" % (H, W, cells, ssim)
                del got, want
                ms, mn = time_ms(lambda: ops.sphere_quality(ref, dist, cells, ssim=ssim, work=work), args.reps, args.warmup)
                tms, tmn = time_ms(lambda: torch_quality(ref, dist, cells, a, ssim), args.torch_reps, 1)
                row = {'frame': [H, W], 'cells': list(cells), 'ssim': ssim, 'video_MB': video / 1e6, 'k26_ms': ms, 'k26_min_ms': mn,
                       'k26_GBps': 2.0 * video / (ms * 1e-3) / 1e9, 'copy_ms': copy_ms, 'copy_min_ms': copy_min, 'copy_GBps': copy_gbps,
                       'torch_ms': tms, 'torch_min_ms': tmn, 'torch_equal': equal}
                rows.append(row)
                lines.append('  cells %3d x %3d  %-10s  K26 %8.3f ms (min %.3f)  %7.1f GB / s read = %.2f of the copy\'s rate   torch %9.3f ms'
                             ' (%.0f x), equal bits' % (cells[0], cells[1], 'sse + ssim' if ssim else 'sse', ms, mn, row['k26_GBps'],
                                                        row['k26_GBps'] / copy_gbps, tms, tms / ms))
                torch.cuda.empty_cache()
        del ref, dist
        torch.cuda.empty_cache()
    ghz = ops.held_clock_ghz()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    head = ['median of %d after %d warm-up calls (HIP events; torch: %d after 1); held clock %.2f GHz, %d CUs'
            % (args.reps, args.warmup, args.torch_reps, ghz, cus)]
    res = {'tool': 'quality_bench', 'frames': F, 'reps': args.reps, 'warmup': args.warmup, 'torch_reps': args.torch_reps,
           'held_clock_ghz': ghz, 'cus': cus, 'rows': rows}
    print('\n'.join(head + lines))
    print(json.dumps(res))
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write('# tools/quality_bench.py on one MI355X\n\n```\n' + '\n'.join(head + lines) + '\n```\n\nThe JSON line of the run:\n\n```\n'
                     + json.dumps(res) + '\n```\n')


if __name__ == '__main__':
    main()
