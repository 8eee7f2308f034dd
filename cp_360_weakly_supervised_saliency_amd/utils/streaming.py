"""Viewport-adaptive streaming (K24, csrc/streaming.hip).  A viewer sees a window of the panorama, so a player should fetch in
high quality the parts that are likely to be in somebody's window.  The model's map is a gaze density; what a player needs is the
expected coverage: how likely a pixel, or a tile, is to be in view.  Source pixel j of the map stands for a viewer whose head
points at its centre (a level camera, ``gaze_cameras``); the window is K17's.  The definitions are the package's own (DESIGN.md
"K24") and tests/streaming_restate.py restates them.

    sp = StreamPlanner()                                       # maps 14 x 28 -> grid 120 x 240, 6 x 12 tiles, 100 degrees square
    cov = sp.coverage(sal)                                     # f32 [F, 120, 240]: compare with HeadMaps.coverage, like with like
    vis = sp.visibility(sal)                                   # f32 [F, 72]: the share of viewers who need the tile
    seg = segment_offsets(F, fps, seconds=1.0, cuts=cuts)
    levels = allocate(sp.demand(vis, seg), sp.area, rates, budget)
    qarea, u = sp.delivered(levels, seg, R, offsets, np.log(rates))          # against the people who watched (head_cameras)
    levels = allocate_measured(demand, bits, dist, budget)     # on a measured rate-distortion table (utils.quality, K26)

The incidence of the windows on the grid depends on the two grids and the window only: a planner computes it once, on first use.
No CPU fallback for the maps and the score; the allocation is host numpy in float64.
"""
import numpy as np
import torch

from .. import ops
from ._device import on_device
from .shots import segments
from .viewport import look_at


def gaze_cameras(src_hw):
    """The camera of every pixel centre of an hs x ws map, in row-major order: float32 [hs ws, 3, 3], ``viewport.look_at`` of
    dir(x, y) (a level camera: a pixel centre is never a pole), formed in float64 and rounded once."""
    hs, ws = (int(v) for v in src_hw)
    if hs < 1 or ws < 1 or hs * ws > ops.STREAM_MAX_SOURCE:
        raise ValueError("the source map must have 1 .. %d pixels, got %d x %d" % (ops.STREAM_MAX_SOURCE, hs, ws))
    theta = (2.0 * (np.arange(ws) + 0.5) / ws - 1.0) * np.pi
    phi = (1.0 - 2.0 * (np.arange(hs) + 0.5) / hs) * (np.pi / 2.0)
    cams = np.empty((hs, ws, 3, 3), np.float64)
    for y in range(hs):
        for x in range(ws):
            cams[y, x] = look_at([np.cos(phi[y]) * np.cos(theta[x]), np.sin(phi[y]), np.cos(phi[y]) * np.sin(theta[x])])
    return np.ascontiguousarray(cams.reshape(hs * ws, 3, 3).astype(np.float32))


def segment_offsets(n_frames, fps, seconds=1.0, cuts=None):
    """The segments a player fetches: int64 [G + 1], segment g holds the frames offsets[g] .. offsets[g + 1] - 1.  Every shot
    (``shots.segments`` of the cuts) is split into segments of round(fps seconds) frames, its last one shorter: a segment never
    straddles a cut."""
    n_frames, fps, seconds = int(n_frames), float(fps), float(seconds)
    if n_frames < 1 or not (fps > 0.0 and np.isfinite(fps)) or not (seconds > 0.0 and np.isfinite(seconds)):
        raise ValueError("n_frames must be at least 1, fps and seconds finite and positive, got %r, %r, %r" % (n_frames, fps, seconds))
    step = max(1, int(round(fps * seconds)))
    edges = [0]
    for lo, hi in segments([] if cuts is None else cuts, n_frames):
        edges.extend(range(lo + step, hi, step))
        edges.append(hi)
    return np.asarray(edges, np.int64)


def _ladder(rates, utility):
    """-> (rates, utility) float64 [L]: rates ascending and positive, the utility (default log(rates)) not decreasing, and the
    slopes du / dr not increasing - the ladder is concave, so that taking the best upgrade first is also the best plan."""
    r = np.asarray(rates, np.float64).reshape(-1)
    if not 1 <= r.size <= ops.STREAM_MAX_LEVELS or not np.all(np.isfinite(r)) or r[0] <= 0.0 or np.any(np.diff(r) <= 0.0):
        raise ValueError("rates must be 1 .. %d finite, positive, ascending values, got %r" % (ops.STREAM_MAX_LEVELS, rates))
    u = np.log(r) if utility is None else np.asarray(utility, np.float64).reshape(-1)
    if u.size != r.size or not np.all(np.isfinite(u)) or np.any(np.diff(u) < 0.0):
        raise ValueError("utility must be %d finite values that do not decrease, got %r" % (r.size, utility))
    slope = np.diff(u) / np.diff(r)
    if np.any(np.diff(slope) > 0.0):
        raise ValueError("the ladder is not concave: its slopes du / dr increase: %r" % (slope.tolist(),))
    return r, u


def _tile_cost(area, r, seconds):
    """cost float64 [T, L]: a tile costs rates[l] area[t] / sum(area) seconds."""
    area = np.asarray(area, np.float64).reshape(-1)
    if area.size < 1 or np.any(area <= 0.0) or not (float(seconds) > 0.0 and np.isfinite(float(seconds))):
        raise ValueError("area must be positive and seconds finite and positive")
    return (area / area.sum())[:, None] * r[None, :] * float(seconds)


def allocate(demand, area, rates, budget, utility=None, seconds=1.0):
    """demand [G, T] (``StreamPlanner.demand``), area [T], rates [L] the ascending bit rates of the whole sphere at every level,
    budget the bits of one segment -> levels int64 [G, T].  Every tile starts at level 0 (ValueError if that alone exceeds the
    budget); then, among the open tiles, the upgrade with the largest demand[t] du / dr is taken, the lowest t on a tie: applied if
    it fits the remaining budget, else the tile is closed; until no tile is open.  Tiles with demand 0 stay at 0."""
    r, u = _ladder(rates, utility)
    cost = _tile_cost(area, r, seconds)
    d = np.asarray(demand.detach().cpu() if torch.is_tensor(demand) else demand, np.float64)
    if d.ndim != 2 or d.shape[1] != cost.shape[0] or not np.all(np.isfinite(d)) or np.any(d < 0.0):
        raise ValueError("demand must be finite, not negative, [G, %d], got %s" % (cost.shape[0], d.shape))
    budget = float(budget)
    if not cost[:, 0].sum() <= budget:
        raise ValueError("every tile at level 0 costs %g, above the budget %g" % (cost[:, 0].sum(), budget))
    L = r.size
    slope = np.append(np.diff(u) / np.diff(r), 0.0)                      # of the upgrade from level l; none from the top
    levels = np.zeros(d.shape, np.int64)
    for g in range(d.shape[0]):
        left = budget - cost[:, 0].sum()
        open_ = (d[g] > 0.0) & (L > 1)
        while open_.any():
            gain = np.where(open_, d[g] * slope[levels[g]], -np.inf)
            t = int(np.argmax(gain))                                   # the first of the largest: the lowest t on a tie
            step = cost[t, levels[g, t] + 1] - cost[t, levels[g, t]]
            if step <= left:
                left -= step
                levels[g, t] += 1
                open_[t] = levels[g, t] < L - 1
            else:
                open_[t] = False
    return levels


def _hull_next(bits, dist):
    """bits, dist float64 [L] -> int64 [L]: from level l the next level along the lower convex hull of the points (bits, dist)
    that starts at level 0 - the higher level with the steepest fall of dist per bit, the lowest on a tie; -1 where every
    higher level has a larger dist (and from the top).  A level of equal dist is a step of gain 0, which ``allocate`` takes too."""
    L = bits.size
    nxt = np.full(L, -1, np.int64)
    for l in range(L - 1):
        slope = (dist[l] - dist[l + 1:]) / (bits[l + 1:] - bits[l])
        k = int(np.argmax(slope))                                      # the first of the largest
        if slope[k] >= 0.0:
            nxt[l] = l + 1 + k
    return nxt


def allocate_measured(demand, bits, dist, budget):
    """``allocate`` on measured tables: demand [G, T], bits float64 [G, T, L] or [T, L] (the bits of the tile at the level,
    ascending in l), dist float64 [G, T, L] (``SphereQuality.rd_table``: the distortion of the tile at the level), budget the
    bits of one segment -> levels int64 [G, T].  The same loop, tie rule and closing rule as ``allocate``; the gain of an upgrade
    is demand[g, t] (dist[from] - dist[to]) / (bits[to] - bits[from]).  Upgrades run along each tile's lower convex hull of
    (bits, dist) from level 0: a level above the hull is skipped, the upgrade goes to the next hull level and costs the sum, so a
    level above the hull is never where a tile ends; a tile whose every higher level is worse is closed (a level that is no
    worse is an upgrade of gain 0, taken while the budget lasts, as ``allocate`` takes an upgrade of slope 0).  Tiles with demand 0 stay
    at 0."""
    d = np.asarray(demand.detach().cpu() if torch.is_tensor(demand) else demand, np.float64)
    dist = np.asarray(dist.detach().cpu() if torch.is_tensor(dist) else dist, np.float64)
    bits = np.asarray(bits.detach().cpu() if torch.is_tensor(bits) else bits, np.float64)
    if dist.ndim != 3 or dist.shape[2] < 1 or not np.all(np.isfinite(dist)):
        raise ValueError("dist must be finite [G, T, L], got %s" % (dist.shape,))
    G, T, L = dist.shape
    if bits.ndim == 2:
        bits = np.broadcast_to(bits[None], (G,) + bits.shape)
    if bits.shape != dist.shape or not np.all(np.isfinite(bits)) or np.any(bits[..., 0] < 0.0) or np.any(np.diff(bits, axis=2) <= 0.0):
        raise ValueError("bits must be finite, not negative and ascending in l, [%d, %d, %d] or [%d, %d], got %s" % (G, T, L, T, L, bits.shape))
    if d.shape != (G, T) or not np.all(np.isfinite(d)) or np.any(d < 0.0):
        raise ValueError("demand must be finite, not negative, [%d, %d], got %s" % (G, T, d.shape))
    budget = float(budget)
    levels = np.zeros((G, T), np.int64)
    for g in range(G):
        base = bits[g, :, 0].sum()
        if not base <= budget:
            raise ValueError("every tile at level 0 costs %g, above the budget %g" % (base, budget))
        nxt = np.stack([_hull_next(bits[g, t], dist[g, t]) for t in range(T)])          # [T, L]
        tiles = np.arange(T)
        to = nxt[tiles, 0]
        left = budget - base
        open_ = (d[g] > 0.0) & (to >= 0)
        while open_.any():
            lv = levels[g]
            safe = np.where(to >= 0, to, lv)
            step = bits[g, tiles, safe] - bits[g, tiles, lv]
            with np.errstate(divide='ignore', invalid='ignore'):
                slope = (dist[g, tiles, lv] - dist[g, tiles, safe]) / step
            gain = np.where(open_, d[g] * slope, -np.inf)
            t = int(np.argmax(gain))                                   # the first of the largest: the lowest t on a tie
            if step[t] <= left:
                left -= step[t]
                levels[g, t] = to[t]
                to[t] = nxt[t, to[t]]
                open_[t] = to[t] >= 0
            else:
                open_[t] = False
    return levels


def uniform(area, rates, budget, seconds=1.0):
    """The highest single level at which every tile fits the budget of a segment (ValueError if none does)."""
    r, _ = _ladder(rates, None)
    total = _tile_cost(area, r, seconds).sum(axis=0)
    fits = np.flatnonzero(total <= float(budget))
    if fits.size == 0:
        raise ValueError("every tile at level 0 costs %g, above the budget %g" % (total[0], float(budget)))
    return int(fits[-1])


def plan_bits(levels, area, rates, seconds=1.0):
    """The bits of every segment of a plan: float64 [G]."""
    r, _ = _ladder(rates, None)
    cost = _tile_cost(area, r, seconds)
    levels = np.asarray(levels, np.int64)
    return cost[np.arange(cost.shape[0])[None, :], levels].sum(axis=1)


class StreamPlanner:
    """``StreamPlanner(grid_hw=(120, 240), src_hw=(14, 28), view_hw=(1, 1), hfov_deg=100.0, tiles=(6, 12))``: from saliency maps to
    the expected coverage of the grid's pixels and tiles, and the quality a tile plan delivers to recorded viewers.  The
    incidence of the gaze cameras' windows on the grid (``inc``, ``tinc``) is built on first use and kept.
    ``resample='conservative'`` brings maps finer than src_hw down by the conservative remap (K25, ``ops.sphere_resample``), which
    keeps their mass on the sphere; the default is the bilinear resampler."""

    def __init__(self, grid_hw=(120, 240), src_hw=(14, 28), view_hw=(1, 1), hfov_deg=100.0, tiles=(6, 12), weights='solid_angle',
                 device='cuda', resample='bilinear'):
        self.resampler = ops.check_resampler(resample)
        h, w, rows, cols = ops._stream_grid(grid_hw, tiles)
        self.grid_hw, self.tiles = (h, w), (rows, cols)
        hs, ws = (int(v) for v in src_hw)
        if hs < 1 or ws < 1 or hs * ws > ops.STREAM_MAX_SOURCE:
            raise ValueError("the source map must have 1 .. %d pixels, got %d x %d" % (ops.STREAM_MAX_SOURCE, hs, ws))
        ops._head_view(view_hw, hfov_deg)
        if weights not in ('solid_angle', 'uniform'):
            raise ValueError("weights must be 'solid_angle' or 'uniform', got %r" % (weights,))
        self.src_hw, self.view_hw, self.hfov_deg = (hs, ws), (float(view_hw[0]), float(view_hw[1])), float(hfov_deg)
        self.weights, self.device = weights, torch.device(device)
        self._inc = self._tinc = self._work = self._area = None

    # ---- the incidence, once
    def _workspace(self, device):
        self._work = ops.view_quality_work(self.grid_hw[0], self.grid_hw[1], device, self._work)
        return self._work

    @property
    def inc(self):
        """int32 [S, ceil(h w / 32)] on the device: ``ops.view_incidence`` of the gaze cameras."""
        if self._inc is None:
            cams = on_device(gaze_cameras(self.src_hw), self.device, torch.float32)
            self._inc = ops.view_incidence(cams, self.grid_hw, self.view_hw, self.hfov_deg, work=self._workspace(cams.device))
        return self._inc

    @property
    def tinc(self):
        """int32 [S, ceil(T / 32)] on the device: ``ops.tile_incidence`` of ``inc``."""
        if self._tinc is None:
            self._tinc = ops.tile_incidence(self.inc, self.grid_hw, self.tiles)
        return self._tinc

    @property
    def area(self):
        """int64 numpy [T]: the sum of the row weights a_y over the tile's pixels, exact."""
        if self._area is None:
            (h, w), (rows, cols) = self.grid_hw, self.tiles
            a = ops.shot_weights_host(h)[0].astype(np.int64) if self.weights == 'solid_angle' else np.full(h, 1024, np.int64)
            per_row = np.zeros(rows, np.int64)
            np.add.at(per_row, (np.arange(h) * rows) // h, a)
            per_col = np.bincount((np.arange(w) * cols) // w, minlength=cols).astype(np.int64)
            self._area = (per_row[:, None] * per_col[None, :]).reshape(-1).astype(np.int64)
        return self._area

    # ---- maps -> coverage
    def _maps(self, sal):
        sal = on_device(sal, self.device, torch.float32)
        if sal.dim() != 3:
            raise ValueError("sal must be [F, hs, ws], got %s" % (tuple(sal.shape),))
        if tuple(sal.shape[1:]) != self.src_hw:
            sal = ops.resample_maps(sal, self.src_hw, self.resampler)
        return sal

    def coverage(self, sal):
        """sal [F, hs', ws'] (maps of another size than src_hw are resampled by ``ops.sphere_eval_resample``, or
        by ``ops.sphere_resample`` with resample='conservative') -> float32 [F, h, w]:
        the expected share of the viewers who have the pixel in view, a viewer's head drawn from the map."""
        sal = self._maps(sal)
        h, w = self.grid_hw
        out, _ = ops.view_expect(sal, ops.sphere_eval_weights(self.src_hw[0], self.weights, sal.device), self.inc, h * w)
        return out.reshape(-1, h, w)

    def visibility(self, sal):
        """-> float32 [F, T]: the expected share of the viewers who have any pixel centre of the tile in view."""
        sal = self._maps(sal)
        return ops.view_expect(sal, ops.sphere_eval_weights(self.src_hw[0], self.weights, sal.device), self.tinc,
                               self.tiles[0] * self.tiles[1])[0]

    @staticmethod
    def demand(vis, seg):
        """vis [F, T], seg int [G + 1] (``segment_offsets``) -> [G, T] on vis's device: the maximum over the segment's frames - a
        tile needed at any moment of a segment must be fetched."""
        seg = [int(v) for v in np.asarray(seg).reshape(-1)]
        if len(seg) < 2 or seg[0] != 0 or seg[-1] != vis.shape[0] or any(b <= a for a, b in zip(seg[:-1], seg[1:])):
            raise ValueError("seg must ascend strictly from 0 to %d, got %r" % (vis.shape[0], seg))
        return torch.stack([vis[a:b].max(dim=0).values for a, b in zip(seg[:-1], seg[1:])])

    # ---- a plan against the people who watched
    def delivered(self, levels, seg, R, offsets, utility):
        """levels int [G, T] (``allocate``), seg int [G + 1], the viewers R, offsets of ``headtrack.head_cameras``, utility [L] ->
        (qarea int64 [N, L] = ``ops.view_quality``, u float64 [N] = sum_l utility[l] qarea[k, l] / sum_l qarea[k, l], the mean
        utility over viewer k's window; NaN for a viewer who sees nothing), both on the device."""
        u = np.asarray(utility, np.float64).reshape(-1)
        seg = np.asarray(seg, np.int64).reshape(-1)
        levels = np.asarray(levels.cpu() if torch.is_tensor(levels) else levels, np.int64)
        if levels.ndim != 2 or levels.shape != (seg.size - 1, self.tiles[0] * self.tiles[1]) or levels.min() < 0:
            raise ValueError("levels must be [%d, %d] and not negative, got %s" % (seg.size - 1, self.tiles[0] * self.tiles[1], levels.shape))
        R = on_device(R, self.device, torch.float32).reshape(-1, 3, 3)
        offsets = on_device(offsets, self.device, torch.int32)
        if int(seg[-1]) != int(offsets.shape[0]) - 1:
            raise ValueError("seg ends at frame %d, the viewers have %d frames" % (int(seg[-1]), int(offsets.shape[0]) - 1))
        per_frame = np.repeat(np.minimum(levels, 255).astype(np.uint8), np.diff(seg), axis=0)
        qarea = ops.view_quality(R, offsets, self.grid_hw, (self.view_hw, self.hfov_deg),
                                 ops.sphere_eval_weights(self.grid_hw[0], self.weights, R.device),
                                 on_device(per_frame, R.device, torch.uint8), self.tiles, u.size, work=self._workspace(R.device))
        q = qarea.to(torch.float64)
        return qarea, (q * torch.from_numpy(u).to(R.device)[None, :]).sum(dim=1) / q.sum(dim=1)

    def evaluate(self, sal, R, offsets, rates, budget, fps, seconds=1.0, cuts=None, utility=None):
        """The plan from the maps, and the uniform plan of the same budget, against the viewers -> {'plan_utility',
        'uniform_utility': the mean delivered utility over the viewers who see anything; 'plan_bits', 'uniform_bits': the mean bits
        of a segment; 'uniform_level', 'levels', 'segments'}."""
        r, u = _ladder(rates, utility)
        vis = self.visibility(sal)
        seg = segment_offsets(vis.shape[0], fps, seconds, cuts)
        levels = allocate(self.demand(vis, seg), self.area, r, budget, u, seconds)
        flat = np.full_like(levels, uniform(self.area, r, budget, seconds))
        res = {'levels': levels, 'segments': seg, 'uniform_level': int(flat[0, 0])}
        for name, lv in (('plan', levels), ('uniform', flat)):
            _, got = self.delivered(lv, seg, R, offsets, u)
            seen = ~torch.isnan(got)
            res[name + '_utility'] = float(got[seen].mean()) if bool(seen.any()) else float('nan')
            res[name + '_bits'] = float(plan_bits(lv, self.area, r, seconds).mean())
        return res
