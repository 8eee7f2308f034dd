"""CPU tests of K26: the restatement (tests/quality_restate.py) against the definition as plain loops, the host tables, the fixed
points of the two sums, the scores of utils/quality.py, ``allocate_measured`` and the entry point's status codes.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from cp_360_weakly_supervised_saliency_amd import _lib, ops
from cp_360_weakly_supervised_saliency_amd.utils import quality, streaming
from tests import quality_restate as qr


def noise(seed, F, H, W):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8), rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)


# ----------------------------------------------------------------------------- the definition
@pytest.mark.parametrize('H,W,cells', [(8, 8, (1, 1)), (8, 12, (2, 3)), (12, 20, (3, 5)), (12, 20, (12, 20))])
def test_restatement_against_the_loops(H, W, cells):
    ref, dist = noise(H + W, 2, H, W)
    sse, q = qr.loops(ref, dist, cells)
    assert np.array_equal(np.array(sse, np.int64), qr.sse(ref, dist, cells))
    assert np.array_equal(np.array(q, np.int64), qr.ssim_q(ref, dist, cells))


@pytest.mark.parametrize('H,W,cells', [(8, 8, (1, 1)), (20, 52, (3, 5)), (24, 40, (6, 10)), (96, 192, (24, 48)), (96, 192, (6, 12)),
                                       (22, 50, (3, 5)), (37, 13, (37, 13))])
def test_host_tables(H, W, cells):
    a = qr.weights(H)
    cw, ww = ops.quality_cell_weights(H, W, cells), ops.quality_window_weights(H, W, cells)
    assert cw.dtype == np.int64 and ww.dtype == np.int64 and cw.shape == ww.shape == (cells[0] * cells[1],)
    assert np.array_equal(cw, qr.cell_weights(H, W, cells)) and np.array_equal(ww, qr.window_weights(H, W, cells))
    assert int(cw.sum()) == W * int(a.sum()) and cw.min() > 0
    if H % 4 == 0 and W % 4 == 0:
        assert int(ww.sum()) == (W // 4) * sum(int(a[4 * i:4 * i + 8].sum()) for i in range(H // 4 - 1))
    else:
        assert not ww.any()
    with pytest.raises(ValueError):
        ops.quality_cell_weights(H, W, (H + 1, 1))
    with pytest.raises(ValueError):
        ops.quality_window_weights(H, W, (1, 0))


@pytest.mark.parametrize('H', [37, 96, 100, 1024])
def test_cells_nest(H):
    y = np.arange(H)
    for r in (1, 2, 3, 6, 7):
        for k in (1, 2, 4, 5):
            if k * r <= H:
                assert np.array_equal(((y * k * r) // H) // k, (y * r) // H)


def test_coarsen():
    H, W = 96, 192
    ref, dist = noise(3, 2, H, W)
    for fn in (qr.sse, qr.ssim_q):
        fine, coarse = fn(ref, dist, (24, 48)), fn(ref, dist, (6, 12))
        assert np.array_equal(quality.coarsen(fine, (24, 48), (6, 12)), coarse)
        assert torch.equal(quality.coarsen(torch.from_numpy(fine), (24, 48), (6, 12)), torch.from_numpy(coarse))
        assert np.array_equal(qr.coarsen(fine, (24, 48), (6, 12)), coarse)
    assert np.array_equal(quality.coarsen(ops.quality_cell_weights(H, W, (24, 48)), (24, 48), (6, 12)), ops.quality_cell_weights(H, W, (6, 12)))
    assert np.array_equal(quality.coarsen(ops.quality_window_weights(H, W, (24, 48)), (24, 48), (6, 12)),
                          ops.quality_window_weights(H, W, (6, 12)))
    for bad in ((5, 12), (6, 10), (48, 48)):
        with pytest.raises(ValueError):
            quality.coarsen(qr.sse(ref, dist, (24, 48)), (24, 48), bad)
    with pytest.raises(ValueError):
        quality.coarsen(np.zeros((2, 7)), (24, 48), (6, 12))


def test_fixed_points():
    H, W, cells = 16, 24, (2, 3)
    ref, _ = noise(5, 2, H, W)
    cw, ww = ops.quality_cell_weights(H, W, cells), ops.quality_window_weights(H, W, cells)
    assert not qr.sse(ref, ref, cells).any()
    assert np.all(qr.window_q(ref, ref) == qr.Q_ONE) and np.array_equal(qr.ssim_q(ref, ref, cells), np.broadcast_to(qr.Q_ONE * ww, (2, 6)))
    black, white = np.zeros_like(ref), np.full_like(ref, 255)
    assert np.array_equal(qr.sse(black, white, cells), np.broadcast_to((65025 * cw)[None, :, None], (2, 6, 3)))
    assert np.all(qr.window_q(black, white) == 26) and np.array_equal(qr.ssim_q(black, white, cells), np.broadcast_to(26 * ww, (2, 6)))
    q = qr.window_q(ref, 255 - ref)
    assert np.all(q < 0) and abs(float(q.mean()) / qr.Q_ONE + 0.96) < 0.05
    assert abs(qr.window_q(ref, ref).max()) <= qr.Q_ONE and int(np.abs(q).max()) <= qr.Q_ONE


# ----------------------------------------------------------------------------- the scores
def test_ws_psnr():
    H, W = 24, 40
    ref, _ = noise(7, 3, H, W)
    ref = np.minimum(ref, 200)
    for d in (1, 7, 55):
        want = 20.0 * math.log10(255.0 / d)
        assert abs(want - qr.ws_psnr_const(d)) == 0.0
        for cells in ((1, 1), (5, 7), (24, 40)):
            sq = quality.SphereQuality(cells=cells, device='cpu', frame_hw=(H, W))
            sse = torch.from_numpy(qr.sse(ref, ref + np.uint8(d), cells))
            for per in ('frame', 'cell', 'video'):
                got = sq.ws_psnr(sse, per=per)
                assert got.dtype == torch.float64 and float((got - want).abs().max()) <= 1e-12 * want, (d, cells, per)
    a, b = noise(8, 2, H, W)
    frame = [quality.SphereQuality(cells=c, device='cpu', frame_hw=(H, W)).ws_psnr(qr.sse(a, b, c)) for c in ((1, 1), (5, 7), (24, 40))]
    assert torch.equal(frame[0], frame[1]) and torch.equal(frame[0], frame[2])          # does not depend on the cells
    sq = quality.SphereQuality(cells=(5, 7), device='cpu', frame_hw=(H, W))
    sse = qr.sse(a, b, (5, 7))
    sse[1] = 0
    sse[0, 3] = 0
    assert torch.isinf(sq.ws_psnr(sse)[1]) and torch.isinf(sq.ws_psnr(sse, per='cell')[0, 3]) and torch.isfinite(sq.ws_psnr(sse)[0])
    with pytest.raises(ValueError):
        sq.ws_psnr(sse, per='tile')
    with pytest.raises(ValueError):
        quality.SphereQuality(cells=(5, 7), device='cpu').ws_psnr(sse)                  # no frame size yet


def test_ws_ssim():
    H, W, cells = 24, 40, (3, 5)
    a, b = noise(9, 2, H, W)
    sq = quality.SphereQuality(cells=cells, device='cpu', frame_hw=(H, W))
    one = sq.ws_ssim(qr.ssim_q(a, a, cells), per='cell')
    assert torch.equal(one, torch.ones_like(one)) and float(sq.ws_ssim(qr.ssim_q(a, a, cells), per='video')) == 1.0
    got = sq.ws_ssim(qr.ssim_q(a, b, cells))
    ww, _ = qr.window_tables(H, W, cells)
    q = qr.window_q(a, b).astype(np.float64) / qr.Q_ONE
    want = (q * ww[None, :, None]).sum(axis=(1, 2)) / (ww.sum() * (W // 4))
    assert np.allclose(got.numpy(), want, rtol=1e-12, atol=0.0)
    top = quality.SphereQuality(cells=(6, 5), device='cpu', frame_hw=(H, W)).ws_ssim(qr.ssim_q(a, b, (6, 5)), per='cell')
    assert bool(torch.isnan(top[:, :5]).all()) and bool(torch.isfinite(top[:, 5:]).all())    # the first cell row holds no window


def test_seen_and_weighted_psnr():
    H, W, cells = 24, 40, (6, 10)
    a, b = noise(10, 3, H, W)
    sq = quality.SphereQuality(cells=cells, device='cpu', frame_hw=(H, W))
    sse = torch.from_numpy(qr.sse(a, b, cells))
    ones = torch.ones((3, 6, 10), dtype=torch.int32)
    assert torch.equal(sq.seen_psnr(sse, ones), sq.ws_psnr(sse, per='frame'))
    assert torch.allclose(sq.weighted_psnr(sse, ones.double()), sq.ws_psnr(sse), rtol=1e-13, atol=0.0)
    assert torch.allclose(sq.weighted_psnr(sse, torch.full((6, 10), 0.25)), sq.ws_psnr(sse), rtol=1e-13, atol=0.0)
    counts = torch.zeros((3, 6, 10), dtype=torch.int32)
    counts[:, 2, 3] = 5
    assert torch.equal(sq.seen_psnr(sse, counts), sq.ws_psnr(sse, per='cell')[:, 23])   # one cell in view: its own PSNR
    assert bool(torch.isnan(sq.seen_psnr(sse, torch.zeros_like(counts))).all())
    with pytest.raises(ValueError):
        sq.seen_psnr(sse * (1 << 40), counts * (1 << 20))
    with pytest.raises(ValueError):
        sq.seen_psnr(sse, counts[:, :5])


def test_plan_sse():
    cells, tiles, F = (6, 8), (3, 2), 5
    rng = np.random.default_rng(11)
    by = torch.from_numpy(rng.integers(0, 1 << 40, (4, F, 48, 3), dtype=np.int64))
    sq = quality.SphereQuality(cells=cells, device='cpu')
    seg = [0, 2, 5]
    for l in range(4):
        assert torch.equal(sq.plan_sse(np.full((2, 6), l), seg, by, tiles), by[l])
    levels = rng.integers(0, 4, (2, 6))
    got = sq.plan_sse(levels, seg, list(by), tiles)
    for f in range(F):
        for r in range(6):
            for c in range(8):
                assert torch.equal(got[f, r * 8 + c], by[levels[0 if f < 2 else 1, (r // 2) * 2 + c // 4], f, r * 8 + c])
    with pytest.raises(ValueError):
        sq.plan_sse(np.full((2, 6), 4), seg, by, tiles)
    with pytest.raises(ValueError):
        sq.plan_sse(levels, seg, by, (4, 2))


# ----------------------------------------------------------------------------- allocate_measured
def ladder(T=8, L=4, seconds=1.0):
    """Tiles of equal area, a power of two of them: ``allocate`` ranks upgrades by du / dr of the whole-sphere ladder and
    ``allocate_measured`` by the tile's own bits, so the two agree where every tile has the same share of the bits - and bit for
    bit where that share is a power of two."""
    rates = np.array([1.0e6, 2.5e6, 6.0e6, 1.6e7][:L])
    area = np.full(T, 5.0)
    return rates, area, np.log(rates), streaming._tile_cost(area, rates, seconds)


def test_allocate_measured_reduces_to_allocate():
    rates, area, u, bits = ladder()
    rng = np.random.default_rng(12)
    for G in (1, 3):
        demand = rng.random((G, 8))
        demand[:, 5] = demand[:, 2]                                    # a tie: the lowest t first
        demand[0, 7] = 0.0
        dist = np.broadcast_to(-u[None, None, :], (G, 8, 4))
        for budget in (rates[0] * 1.000001, rates[1] * 1.3, rates[3] * 2.0):
            want = streaming.allocate(demand, area, rates, budget, u)
            got = streaming.allocate_measured(demand, bits, dist, budget)
            assert got.dtype == np.int64 and np.array_equal(got, want), budget
            assert np.array_equal(streaming.allocate_measured(demand, np.broadcast_to(bits, (G, 8, 4)), dist, budget), want)
            assert np.all(bits[np.arange(8)[None, :], got].sum(axis=1) <= budget)
    assert want.max() == 3 and want[0, 7] == 0                         # the last budget buys everything; demand 0 stays at 0
    rates2, area2, u2, bits2 = ladder(seconds=2.0)
    demand = rng.random((2, 8))
    assert np.array_equal(streaming.allocate_measured(demand, bits2, np.broadcast_to(-u2, (2, 8, 4)), 5.0e6),
                          streaming.allocate(demand, area2, rates2, 5.0e6, u2, 2.0))


def test_allocate_measured_departs_from_allocate_on_unequal_areas():
    """What ``ladder`` says, pinned: ``allocate`` ranks by demand du / dr and ``allocate_measured`` by the tile's own bits, so with
    areas 1 : 3 a small tile in lower demand is upgraded first by the one and last by the other."""
    rates, area, u, demand = np.array([1.0, 2.0]), np.array([1.0, 3.0]), np.array([0.0, 1.0]), np.array([[1.0, 1.5]])
    bits = streaming._tile_cost(area, rates, 1.0)
    assert bits.tolist() == [[0.25, 0.5], [0.75, 1.5]]
    dist = np.broadcast_to(-u, (1, 2, 2))
    assert streaming.allocate(demand, area, rates, 1.75, u).tolist() == [[0, 1]]          # gains 1 and 1.5: the large tile, 0.75 bits
    assert streaming.allocate_measured(demand, bits, dist, 1.75).tolist() == [[1, 0]]     # gains 4 and 2: the small tile, 0.25 bits
    for budget in (1.0, 2.0):                                                              # nothing or everything: the same
        assert np.array_equal(streaming.allocate_measured(demand, bits, dist, budget), streaming.allocate(demand, area, rates, budget, u))


def test_allocate_measured_stays_within_the_budget():
    rng = np.random.default_rng(13)
    for _ in range(20):
        G, T, L = 2, 7, 5
        bits = np.cumsum(rng.random((G, T, L)) + 0.1, axis=2)
        dist = rng.random((G, T, L)) * 10.0                            # not monotone, not convex
        demand = rng.random((G, T)) * (rng.random((G, T)) > 0.2)
        budget = bits[:, :, 0].sum(axis=1).max() + rng.random() * 10.0
        lv = streaming.allocate_measured(demand, bits, dist, budget)
        spent = np.take_along_axis(bits, lv[:, :, None], 2)[:, :, 0].sum(axis=1)
        assert np.all(spent <= budget) and np.all(lv[demand == 0.0] == 0)


def test_allocate_measured_walks_the_hull():
    """The rule: a tile only ever stands on a level of the lower convex hull of its (bits, dist) points that starts at level 0; a
    level above the hull is passed over in one upgrade that costs the sum, and is never where a tile ends - the top level
    included, which is reached only where it is on the hull."""
    bits = np.array([[1.0, 2.0, 3.0, 4.0]])
    dist = np.array([[[10.0, 9.5, 4.0, 3.9]]])                         # level 1 lies above the chord from 0 to 2
    assert streaming._hull_next(bits[0], dist[0, 0]).tolist() == [2, 2, 3, -1]
    demand = np.ones((1, 1))
    for budget, want in ((1.0, 0), (2.0, 0), (2.9, 0), (3.0, 2), (3.9, 2), (4.0, 3)):
        assert streaming.allocate_measured(demand, bits, dist, budget).tolist() == [[want]], budget
    dist = np.array([[[10.0, 4.0, 5.0, 6.0]]])                         # nothing above level 1 helps: the tile closes there
    assert streaming.allocate_measured(demand, bits, dist, 100.0).tolist() == [[1]]
    dist = np.array([[[10.0, 4.0, 4.0, 6.0]]])                         # a level that neither helps nor harms is taken, as
    assert streaming.allocate_measured(demand, bits, dist, 100.0).tolist() == [[2]]    # ``allocate`` takes an upgrade of slope 0
    dist = np.array([[[10.0, 9.0, 8.0, 7.0]]])                         # a straight line: level by level, the nearest first
    assert streaming._hull_next(bits[0], dist[0, 0]).tolist() == [1, 2, 3, -1]
    assert streaming.allocate_measured(demand, bits, dist, 2.5).tolist() == [[1]]


def test_allocate_measured_refusals():
    bits = np.array([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0]])
    dist = np.zeros((1, 2, 3))
    demand = np.ones((1, 2))
    assert streaming.allocate_measured(demand, bits, dist, 2.0).shape == (1, 2)
    for bad in (np.array([[1.0, 2.0, 2.0], [1.0, 2.0, 3.0]]), np.array([[1.0, 3.0, 2.0], [1.0, 2.0, 3.0]]),
                np.array([[1.0, 2.0, np.inf], [1.0, 2.0, 3.0]]), np.array([[1.0, 2.0, np.nan], [1.0, 2.0, 3.0]]), bits[:1]):
        with pytest.raises(ValueError):
            streaming.allocate_measured(demand, bad, dist, 2.0)
    for bad in (np.full((1, 2, 3), np.nan), np.full((1, 2, 3), np.inf), np.zeros((2, 3))):
        with pytest.raises(ValueError):
            streaming.allocate_measured(demand, bits, bad, 2.0)
    for bad in (-demand, demand * np.nan, np.ones((2, 2))):
        with pytest.raises(ValueError):
            streaming.allocate_measured(bad, bits, dist, 2.0)
    with pytest.raises(ValueError):
        streaming.allocate_measured(demand, bits, dist, 1.9)           # level 0 above the budget


# ----------------------------------------------------------------------------- the entry point
def test_status_codes_without_gpu():
    L = _lib.lib()
    one, big = C.c_void_p(16), 1 << 20
    call = L.cp360_sphere_quality
    assert call(one, one, 1, 16, 32, 2, 4, one, one, one, one, big, None) != -5
    for k in (0, 1, 7, 8, 10):                                         # ref, dist, weights, sse, work; ssim_q may be NULL
        args = [one, one, 1, 16, 32, 2, 4, one, one, one, one, big, None]
        args[k] = None
        assert call(*args) == -5, k
    assert call(None, one, 0, 16, 32, 2, 4, one, one, one, one, big, None) == -5        # NULL comes first
    for F, H, W, rows, cols in ((0, 16, 32, 2, 4), (1, 0, 32, 1, 4), (1, 16, 32, 17, 4), (1, 16, 32, 2, 33), (1, 16, 32, 0, 4),
                                (1, 16, 32, 2, 0)):
        assert call(one, one, F, H, W, rows, cols, one, one, None, one, big, None) == -1, (F, H, W, rows, cols)
    for H, W in ((18, 32), (16, 30), (4, 32), (16, 4)):
        assert call(one, one, 1, H, W, 1, 1, one, one, one, one, big, None) == -1, (H, W)             # ssim_q asked for
        assert call(one, one, 1, H, W, 1, 1, one, C.c_void_p(20), None, one, big, None) == -6, (H, W)  # the squared error alone: next check
    assert call(one, one, 70000, 16, 32, 2, 4, C.c_void_p(20), one, one, one, big, None) == -8        # unsupported before alignment
    assert call(one, one, 1, 16, 1 << 22, 2, 4, one, one, one, one, big, None) == -8
    for k, p in ((8, 20), (9, 20), (7, 18), (10, 24)):                 # sse, ssim_q 8 bytes, weights 4, work 16
        args = [one, one, 1, 16, 32, 2, 4, one, one, one, one, 0, None]
        args[k] = C.c_void_p(p)
        assert call(*args) == -6, k
    need = L.cp360_sphere_quality_work_bytes(1, 16, 32, 2, 4)
    assert need > 0 and need % 16 == 0
    assert call(one, one, 1, 16, 32, 2, 4, one, one, one, one, need - 1, None) == -1
    assert L.cp360_sphere_quality_work_bytes(1, 16, 32, 17, 4) == 0 and L.cp360_sphere_quality_work_bytes(70000, 16, 32, 2, 4) == 0
    assert L.cp360_sphere_quality_work_bytes(1, 18, 30, 2, 4) > 0      # the squared error has no demand on the size


def test_ops_refuse_without_gpu():
    ref = torch.zeros((1, 8, 8, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        ops.sphere_quality(ref, ref, (1, 1))
    with pytest.raises(ValueError):
        quality.SphereQuality(cells=(0, 1), device='cpu')
