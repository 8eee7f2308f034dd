"""Video quality on the sphere (K26, csrc/sphere_quality.hip): how good a decoded video is against its source - on the whole
sphere (WS-PSNR, WS-SSIM), in each cell or tile, and in what recorded viewers had in view.  The definitions are the package's own
(DESIGN.md "K26", 7r) and tests/quality_restate.py restates them.  Encoding and decoding stay the caller's job.

    sq = SphereQuality()                                       # cells 120 x 240: the grid of K17's footprints and K24's coverage
    m = sq.measure(ref, dist)                                  # {'sse': int64 [F, T, 3], 'ssim_q': int64 [F, T]} on the device
    sq.ws_psnr(m['sse']), sq.ws_ssim(m['ssim_q'])              # float64 [F]
    sq.seen_psnr(m['sse'], counts)                             # counts = ops.head_footprints on the same cells
    dist = sq.rd_table(ref, encodes, seg)                      # float64 [G, 72, L]: the WS-MSE of tile t in segment g at level l
    levels = allocate_measured(demand, bits, dist, budget)     # utils.streaming
    sq.seen_psnr(sq.plan_sse(levels, seg, sse_by_level, (6, 12)), counts)     # the plan against the people who watched

One measurement on fine cells also gives every coarser grid that nests in them (``coarsen``): the sums are exact integers.
No CPU fallback for the measurement; the scores are float64 formed from the int64 sums, on the sums' device.
"""
import numpy as np
import torch

from .. import ops
from ._device import host_tensor, on_device

Q_ONE = 1 << 24                                                        # q = 2^24: a window of identical pixels
PEAK2 = 255.0 * 255.0


def _nest(cells, to_cells):
    (r, c), (R, Cc) = ((int(v) for v in cells), (int(v) for v in to_cells))
    if min(r, c, R, Cc) < 1 or r % R != 0 or c % Cc != 0:
        raise ValueError("cells %r do not nest in %r: the rows and the columns must be multiples" % (tuple(cells), tuple(to_cells)))
    return r, c, R, Cc


def coarsen(x, cells, to_cells, axis=None):
    """x [.., rows cols] or [.., rows cols, 3] on `cells` -> the same on `to_cells`, every fine cell added to the coarse cell it
    lies in.  Exact for integers.  ValueError unless rows and cols are multiples of to_cells' (then every fine cell of any frame
    lies in one coarse cell).  axis: the cell axis, by default -2 for a [.., rows cols, 3] array, else -1."""
    r, c, R, Cc = _nest(cells, to_cells)
    t = host_tensor(x)
    if axis is None:
        axis = -2 if t.dim() >= 2 and t.shape[-1] == 3 and t.shape[-2] == r * c else -1
    axis = axis % t.dim()
    if t.shape[axis] != r * c:
        raise ValueError("x has %d cells on axis %d, cells %r have %d" % (t.shape[axis], axis, tuple(cells), r * c))
    lead, tail = tuple(t.shape[:axis]), tuple(t.shape[axis + 1:])
    n = len(lead)
    out = t.reshape(lead + (R, r // R, Cc, c // Cc) + tail).sum(dim=(n + 1, n + 3)).reshape(lead + (R * Cc,) + tail)
    return out if torch.is_tensor(x) else out.numpy()


def _cell_to_tile(cells, tiles):
    """int64 [rows cols]: the tile of every cell."""
    r, c, R, Cc = _nest(cells, tiles)
    return ((np.arange(r) // (r // R))[:, None] * Cc + (np.arange(c) // (c // Cc))[None, :]).reshape(-1).astype(np.int64)


def _segments(seg, F):
    seg = [int(v) for v in np.asarray(seg).reshape(-1)]
    if len(seg) < 2 or seg[0] != 0 or seg[-1] != F or any(b <= a for a, b in zip(seg[:-1], seg[1:])):
        raise ValueError("seg must ascend strictly from 0 to %d, got %r" % (F, seg))
    return seg


def _psnr(num, den):
    return 10.0 * torch.log10(num / den)


class SphereQuality:
    """``SphereQuality(cells=(120, 240), device='cuda', resample='bilinear')``: the measurement of two videos on `cells`, and the
    scores formed from it.  The frame size is the one of the last ``measure`` (or ``frame_hw=``); the weights of its cells and
    windows are host tables (``ops.quality_cell_weights``, ``ops.quality_window_weights``), kept per frame size."""

    def __init__(self, cells=(120, 240), device='cuda', resample='bilinear', frame_hw=None):
        rows, cols = (int(v) for v in cells)
        if rows < 1 or cols < 1:
            raise ValueError("cells must be at least 1 x 1, got %r" % (tuple(cells),))
        self.cells, self.device = (rows, cols), torch.device(device)
        self.resampler = ops.check_resampler(resample)
        self.frame_hw = None if frame_hw is None else (int(frame_hw[0]), int(frame_hw[1]))
        self._work, self._tables = None, {}

    # ---- tables
    def _hw(self, hw):
        hw = self.frame_hw if hw is None else (int(hw[0]), int(hw[1]))
        if hw is None:
            raise ValueError("the frame size is not known yet: measure first, or pass hw=(H, W)")
        return hw

    def cell_weights(self, hw=None, cells=None):
        """int64 numpy [T]: the sum of a_y over the cell's pixels."""
        key = ('c', self._hw(hw), self.cells if cells is None else tuple(int(v) for v in cells))
        if key not in self._tables:
            self._tables[key] = ops.quality_cell_weights(key[1][0], key[1][1], key[2])
        return self._tables[key]

    def window_weights(self, hw=None, cells=None):
        """int64 numpy [T]: the sum of ww over the cell's windows; 0 for a cell without one."""
        key = ('w', self._hw(hw), self.cells if cells is None else tuple(int(v) for v in cells))
        if key not in self._tables:
            self._tables[key] = ops.quality_window_weights(key[1][0], key[1][1], key[2])
        return self._tables[key]

    # ---- measuring
    def measure(self, ref, dist, ssim=True):
        """ref, dist uint8 [F, H, W, 3] -> {'sse': int64 [F, T, 3], 'ssim_q': int64 [F, T] or None} on the device."""
        ref, dist = on_device(ref, self.device), on_device(dist, self.device)
        if ref.dim() != 4:
            raise ValueError("ref must be uint8 [F, H, W, 3], got %s" % (tuple(ref.shape),))
        F, H, W = (int(v) for v in ref.shape[:3])
        self._work = ops.sphere_quality_work(F, H, W, self.cells, ref.device, self._work)
        sse, ssim_q = ops.sphere_quality(ref, dist, self.cells, ssim=ssim, work=self._work)
        self.frame_hw = (H, W)
        return {'sse': sse, 'ssim_q': ssim_q}

    def to_cells(self, maps):
        """maps float [F, hs, ws] -> float32 [F, rows, cols] on the device by the class's resampler."""
        maps = on_device(maps, self.device, torch.float32)
        return maps if tuple(maps.shape[1:]) == self.cells else ops.resample_maps(maps, self.cells, self.resampler)

    # ---- scores
    def _sse(self, sse, cells):
        sse = host_tensor(sse)
        T = (self.cells if cells is None else cells)[0] * (self.cells if cells is None else cells)[1]
        if sse.dim() != 3 or sse.shape[1] != T or sse.shape[2] != 3 or sse.dtype != torch.int64:
            raise ValueError("sse must be int64 [F, %d, 3], got %s %s" % (T, sse.dtype, tuple(sse.shape)))
        return sse

    def ws_psnr(self, sse, per='frame', hw=None, cells=None):
        """10 log10(255^2 3 sum(weights) / sum_c sse) in float64: per='frame' [F], 'cell' [F, T] or 'video' (a scalar tensor); inf
        where the error is 0."""
        sse = self._sse(sse, cells)
        w = torch.from_numpy(self.cell_weights(hw, cells)).to(sse.device)
        e = sse.sum(dim=2)
        if per == 'cell':
            return _psnr(PEAK2 * 3.0 * w.to(torch.float64)[None, :], e.to(torch.float64))
        if per == 'frame':
            den = e.sum(dim=1).to(torch.float64)
            return _psnr(torch.full_like(den, PEAK2 * 3.0 * float(int(w.sum()))), den)
        if per == 'video':
            return _psnr(torch.tensor(PEAK2 * 3.0 * float(int(w.sum()) * int(sse.shape[0])), dtype=torch.float64, device=sse.device),
                         e.sum().to(torch.float64))
        raise ValueError("per must be 'frame', 'cell' or 'video', got %r" % (per,))

    def ws_ssim(self, ssim_q, per='frame', hw=None, cells=None):
        """ssim_q / (2^24 window weights) in float64, per as in ``ws_psnr``; NaN for a cell without a window."""
        q = host_tensor(ssim_q)
        ww = torch.from_numpy(self.window_weights(hw, cells)).to(q.device)
        if q.dim() != 2 or q.shape[1] != ww.shape[0] or q.dtype != torch.int64:
            raise ValueError("ssim_q must be int64 [F, %d], got %s %s" % (ww.shape[0], q.dtype, tuple(q.shape)))
        if per == 'cell':
            return q.to(torch.float64) / (float(Q_ONE) * ww.to(torch.float64))[None, :]
        if per == 'frame':
            return q.sum(dim=1).to(torch.float64) / (float(Q_ONE) * float(int(ww.sum())))
        if per == 'video':
            return q.sum().to(torch.float64) / (float(Q_ONE) * float(int(ww.sum()) * int(q.shape[0])))
        raise ValueError("per must be 'frame', 'cell' or 'video', got %r" % (per,))

    def seen_psnr(self, sse, counts, hw=None):
        """Viewport PSNR: sse int64 [F, T, 3], counts int32 [F, rows, cols] (``ops.head_footprints`` on the cells: how many
        recorded viewers had the cell in view) -> float64 [F]: 10 log10(255^2 3 sum(counts weights) / sum(counts sse)), the sums
        in int64.  NaN for a frame nobody watched."""
        sse = self._sse(sse, None)
        counts = host_tensor(counts).to(sse.device)
        if tuple(counts.shape) != (sse.shape[0],) + self.cells or counts.dtype not in (torch.int32, torch.int64):
            raise ValueError("counts must be int32 [%d, %d, %d], got %s %s" % ((sse.shape[0],) + self.cells + (counts.dtype, tuple(counts.shape))))
        n = counts.reshape(sse.shape[0], -1).to(torch.int64)
        e = sse.sum(dim=2)
        w = torch.from_numpy(self.cell_weights(hw)).to(sse.device)
        top = int(n.max()) if n.numel() else 0
        if int(n.min()) < 0 or int(e.min()) < 0 or top * max(int(e.max()), int(w.max())) * n.shape[1] >= 1 << 63:
            raise ValueError("counts must not be negative, and max(counts) max(sse) cells must stay below 2^63")
        return _psnr(PEAK2 * 3.0 * (n * w[None, :]).sum(dim=1).to(torch.float64), (n * e).sum(dim=1).to(torch.float64))

    def weighted_psnr(self, sse, maps, hw=None):
        """The same with a float map per cell, [F, rows, cols] or [rows, cols] (``StreamPlanner.coverage``, ``HeadMaps.coverage``,
        a saliency map from ``to_cells``), in float64 -> [F]."""
        sse = self._sse(sse, None)
        m = host_tensor(maps).to(sse.device, torch.float64)
        if m.dim() == 2:
            m = m[None].expand(sse.shape[0], -1, -1)
        if tuple(m.shape) != (sse.shape[0],) + self.cells:
            raise ValueError("maps must be [%d, %d, %d] or [%d, %d], got %s" % ((sse.shape[0],) + self.cells + self.cells + (tuple(m.shape),)))
        m = m.reshape(sse.shape[0], -1)
        w = torch.from_numpy(self.cell_weights(hw)).to(sse.device, torch.float64)
        return _psnr(PEAK2 * 3.0 * (m * w[None, :]).sum(dim=1), (m * sse.sum(dim=2).to(torch.float64)).sum(dim=1))

    # ---- rate-distortion tables, and the video a plan delivers
    def rd_table(self, ref, encodes, seg, tiles=(6, 12)):
        """ref uint8 [F, H, W, 3], encodes a sequence of L decoded videos of ref's shape, lowest level first, seg int [G + 1]
        (``segment_offsets``) -> float64 numpy [G, T, L]: the WS-MSE of tile t in segment g at level l, the squared error summed
        over the segment's frames and the channels / (3 frames the tile's weight).  Measured on the class's cells, one level at a
        time (one workspace), and coarsened."""
        ref = on_device(ref, self.device)
        seg = _segments(seg, int(ref.shape[0]))
        _nest(self.cells, tiles)
        per_level = []
        for enc in encodes:
            e = coarsen(self.measure(ref, enc, ssim=False)['sse'], self.cells, tiles).sum(dim=2)          # int64 [F, T]
            per_level.append(torch.stack([e[a:b].sum(dim=0) for a, b in zip(seg[:-1], seg[1:])]))
        if not per_level:
            raise ValueError("encodes must hold at least one video")
        e = torch.stack(per_level, dim=2).cpu().numpy().astype(np.float64)                                # [G, T, L]
        w = self.cell_weights(cells=tiles).astype(np.float64)
        frames = np.diff(np.asarray(seg, np.int64)).astype(np.float64)
        return e / (3.0 * frames[:, None, None] * w[None, :, None])

    def plan_sse(self, levels, seg, sse_by_level, tiles=(6, 12)):
        """levels int [G, T] (``allocate_measured``), seg int [G + 1], sse_by_level int64 [L, F, cells, 3] (or a sequence of L
        measurements) -> int64 [F, cells, 3]: the squared error of the video the plan delivers - every cell takes the level of
        its tile in its frame's segment."""
        by = sse_by_level if torch.is_tensor(sse_by_level) else torch.stack([host_tensor(s) for s in sse_by_level])
        if by.dim() != 4 or by.shape[2] != self.cells[0] * self.cells[1] or by.shape[3] != 3:
            raise ValueError("sse_by_level must be [L, F, %d, 3], got %s" % (self.cells[0] * self.cells[1], tuple(by.shape)))
        L, F = int(by.shape[0]), int(by.shape[1])
        seg = _segments(seg, F)
        tile = _cell_to_tile(self.cells, tiles)
        levels = np.asarray(levels.cpu() if torch.is_tensor(levels) else levels, np.int64)
        if levels.shape != (len(seg) - 1, int(tiles[0]) * int(tiles[1])) or levels.min() < 0 or levels.max() >= L:
            raise ValueError("levels must be [%d, %d] in 0 .. %d, got %s" % (len(seg) - 1, int(tiles[0]) * int(tiles[1]), L - 1, levels.shape))
        per_frame = np.repeat(levels, np.diff(np.asarray(seg, np.int64)), axis=0)[:, tile]                # [F, cells]
        idx = torch.from_numpy(per_frame).to(by.device)[None, :, :, None].expand(1, F, by.shape[2], 3)
        return torch.gather(by, 0, idx)[0]
