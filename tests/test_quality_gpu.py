"""GPU tests of K26 (csrc/sphere_quality.hip, utils/quality.py): the weighted squared error and the windowed structural similarity
per cell, bit for bit against tests/quality_restate.py on every launch path, and the class end to end on K17's scene."""
import functools

import numpy as np
import pytest
import torch

from cp_360_weakly_supervised_saliency_amd import ops
from cp_360_weakly_supervised_saliency_amd.utils import headtrack, quality, streaming
from tests import quality_restate as qr

pytestmark = pytest.mark.gpu

# (H, W, cells, with the structural similarity)
CASES = {
    'one_cell': (8, 8, (1, 1), True),
    'pixel_cells': (8, 16, (8, 16), True),                  # one pixel per cell: many cells per vector
    'nothing_divides': (20, 52, (3, 5), True),              # rows of 156 bytes
    'no_windows': (22, 50, (3, 5), False),                  # rows of 150 bytes, a last block of 2 columns and of 2 rows
    'odd_cells': (24, 40, (5, 7), True),
    'fine': (96, 192, (24, 48), True),
    'tiles': (96, 192, (6, 12), True),
    'three_cells_a_vector': (16, 48, (2, 40), True),
    'split_cell_row': (600, 64, (2, 3), True),              # a cell row over several workgroups
    'wide': (64, 2048, (3, 240), True),                     # several workgroups per row
}
F = 3


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()


@functools.lru_cache(maxsize=None)
def videos(H, W, n=F):
    rng = np.random.default_rng(26 + H * 7 + W)
    ref = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    dist = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    dist[1] = ref[1]                                         # one frame pair identical
    ref.setflags(write=False), dist.setflags(write=False)
    return ref, dist


@functools.lru_cache(maxsize=None)
def want(name):
    H, W, cells, ssim = CASES[name]
    ref, dist = videos(H, W)
    return qr.sse(ref, dist, cells), (qr.ssim_q(ref, dist, cells) if ssim else None)


@functools.lru_cache(maxsize=None)
def got(name):
    H, W, cells, ssim = CASES[name]
    ref, dist = videos(H, W)
    sse, q = ops.sphere_quality(dev(ref), dev(dist), cells, ssim=ssim)
    return sse.cpu().numpy(), (q.cpu().numpy() if ssim else None)


@pytest.mark.parametrize('name', sorted(CASES))
def test_sse_exact(name):
    sse = got(name)[0]
    assert sse.dtype == np.int64 and np.array_equal(sse, want(name)[0])
    assert not sse[1].any() and sse[0].any() and sse[2].any()


@pytest.mark.parametrize('name', sorted(n for n in CASES if CASES[n][3]))
def test_ssim_exact(name):
    H, W, cells, _ = CASES[name]
    q = got(name)[1]
    assert q.dtype == np.int64 and np.array_equal(q, want(name)[1])
    assert np.array_equal(q[1], qr.Q_ONE * ops.quality_window_weights(H, W, cells))


def test_fine_cells_coarsen_to_the_tiles():
    for k in (0, 1):
        fine, tiles = got('fine')[k], got('tiles')[k]
        assert np.array_equal(quality.coarsen(fine, (24, 48), (6, 12)), tiles)
        assert torch.equal(quality.coarsen(dev(fine), (24, 48), (6, 12)).cpu(), torch.from_numpy(tiles))


@pytest.mark.parametrize('name', ['odd_cells', 'nothing_divides', 'no_windows'])
def test_frames_at_any_byte(name):
    H, W, cells, ssim = CASES[name]
    ref, dist = videos(H, W)
    n = ref.size
    for o_ref, o_dist in ((1, 5), (5, 16), (16, 1)):
        a, b = torch.zeros(n + 32, dtype=torch.uint8, device='cuda'), torch.zeros(n + 32, dtype=torch.uint8, device='cuda')
        a[o_ref:o_ref + n] = dev(ref).reshape(-1)
        b[o_dist:o_dist + n] = dev(dist).reshape(-1)
        sse, q = ops.sphere_quality(a[o_ref:o_ref + n].view(ref.shape), b[o_dist:o_dist + n].view(ref.shape), cells, ssim=ssim)
        assert np.array_equal(sse.cpu().numpy(), got(name)[0]), (o_ref, o_dist)
        assert not ssim or np.array_equal(q.cpu().numpy(), got(name)[1]), (o_ref, o_dist)


@pytest.mark.parametrize('H,W,cells', [(512, 64, (1, 1)), (64, 4096, (1, 2))])
def test_black_against_white(H, W, cells):
    """The widest sums a narrow accumulator meets: every term is 65025 a_y."""
    ref = torch.zeros((2, H, W, 3), dtype=torch.uint8, device='cuda')
    dist = torch.full((2, H, W, 3), 255, dtype=torch.uint8, device='cuda')
    sse, q = ops.sphere_quality(ref, dist, cells)
    cw, ww = ops.quality_cell_weights(H, W, cells), ops.quality_window_weights(H, W, cells)
    assert np.array_equal(sse.cpu().numpy(), np.broadcast_to((65025 * cw)[None, :, None], (2, cw.size, 3)))
    assert np.array_equal(q.cpu().numpy(), np.broadcast_to((26 * ww)[None, :], (2, ww.size)))


def test_seam_and_last_rows():
    """Columns W - 4 .. W - 1 lie in the windows j = W / 4 - 2 and W / 4 - 1 (the last one wraps), rows H - 4 .. H - 1 in the
    window row H / 4 - 2 alone.  One window per cell: cells (H / 4, W / 4) on a frame whose cells are blocks."""
    H, W = 24, 40
    cells = (H // 4, W // 4)
    ref, dist = videos(H, W)
    base = ops.sphere_quality(dev(ref), dev(dist), cells)[1].cpu().numpy().reshape(F, H // 4, W // 4)
    d2 = dist.copy()
    d2[:, :, W - 4:] ^= 0x55
    q2 = ops.sphere_quality(dev(ref), dev(d2), cells)[1].cpu().numpy().reshape(F, H // 4, W // 4)
    assert np.array_equal(q2.reshape(F, -1), qr.ssim_q(ref, d2, cells))
    # window (i, j) lies in cell (i + 1, (j + 1) % (W / 4)): the windows j = W / 4 - 2, W / 4 - 1 are the cell columns W / 4 - 1, 0
    changed = (q2 != base).any(axis=(0, 1))
    assert changed.tolist() == [True] + [False] * (W // 4 - 2) + [True]
    d3 = dist.copy()
    d3[:, H - 4:] ^= 0x55
    q3 = ops.sphere_quality(dev(ref), dev(d3), cells)[1].cpu().numpy().reshape(F, H // 4, W // 4)
    assert np.array_equal(q3.reshape(F, -1), qr.ssim_q(ref, d3, cells))
    assert (q3 != base).any(axis=(0, 2)).tolist() == [False] * (H // 4 - 1) + [True]


def test_without_ssim():
    """ssim=False returns None and the same squared error, and takes frames that have no windows.  20 x 52 has windows by the
    definition (both are multiples of 4), so it is measured in full above; 22 x 50 is the frame that ssim=True refuses."""
    for name in ('odd_cells', 'nothing_divides', 'no_windows'):
        H, W, cells, _ = CASES[name]
        ref, dist = videos(H, W)
        sse, q = ops.sphere_quality(dev(ref), dev(dist), cells, ssim=False)
        assert q is None and np.array_equal(sse.cpu().numpy(), got(name)[0])
    ref, dist = videos(22, 50)
    for r, d in ((ref, dist), (ref[:, :20], dist[:, :20]), (ref[:, :, :48], dist[:, :, :48]), (ref[:, :4, :48], dist[:, :4, :48])):
        with pytest.raises(ValueError):                                # before any launch
            ops.sphere_quality(dev(r), dev(d), (3, 5), ssim=True)


def test_a_frame_does_not_depend_on_the_batch():
    H, W, cells, _ = CASES['odd_cells']
    ref, dist = videos(H, W, 5)
    sse, q = ops.sphere_quality(dev(ref), dev(dist), cells)
    for f in range(5):
        s1, q1 = ops.sphere_quality(dev(ref[f:f + 1]), dev(dist[f:f + 1]), cells)
        assert torch.equal(s1[0], sse[f]) and torch.equal(q1[0], q[f])


def test_workspace():
    H, W, cells, _ = CASES['tiles']
    ref, dist = (dev(v) for v in videos(H, W))
    work = ops.sphere_quality_work(F, H, W, cells, ref.device)
    assert ops.sphere_quality_work(F, H, W, cells, ref.device, work) is work
    for _ in range(2):                                                 # repeatable with a caller's workspace
        sse, q = ops.sphere_quality(ref, dist, cells, work=work)
        assert np.array_equal(sse.cpu().numpy(), got('tiles')[0]) and np.array_equal(q.cpu().numpy(), got('tiles')[1])
    with pytest.raises(ValueError):
        ops.sphere_quality(ref, dist, cells, work=work[:4])
    with pytest.raises(ValueError):
        ops.sphere_quality(ref, dist[:2], cells)
    with pytest.raises(RuntimeError):
        ops.sphere_quality(ref.cpu(), dist.cpu(), cells)


# ----------------------------------------------------------------------------- the bands of a full video
def band_rows(n, H, W, cells):
    """The block rows of a workgroup's band as csrc/sphere_quality.hip's quality_geom chooses them: 32, halved while the launch
    has fewer than 1024 workgroups, 4 at least.  Few small frames always end at 4 (16 pixel rows): the shapes below keep more."""
    nb, nbr = (W + 3) // 4, (H + 3) // 4
    cwmax = 256 if W // cells[1] >= 4 else 64
    chunks = -(-nb // cwmax)
    chunks = -(-nb // -(-nb // chunks))
    band = 32
    while band > 4 and n * chunks * -(-nbr // band) < 1024:
        band //= 2
    return band


# (frames, H, W, cells, the band it keeps)
LONG = {
    'band32_one_band': (1024, 128, 8, (1, 1), 32),          # 128 rows of one cell in one workgroup: four flushes of 32 rows
    'band32_halo': (1024, 256, 8, (3, 2), 32),              # two bands: the halo is 1 / 32; cell rows end inside a band, 85 rows each
    'band16': (256, 256, 8, (5, 1), 16),                    # four bands of 64 rows, cell rows of 51 end inside them
}


@functools.lru_cache(maxsize=None)
def long_videos(name):
    n, H, W, _, _ = LONG[name]
    rng = np.random.default_rng(sum(name.encode()))
    ref = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    dist = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    dist[:, :64, :4] = 255 - (ref[:, :64, :4] >> 7) * 255    # 64 rows of a column block with errors of 128 .. 255
    return ref, dist


@pytest.mark.parametrize('name', sorted(LONG))
def test_long_bands_exact(name):
    """The launch of a whole video: bands of 32 and of 16 block rows, where a thread's u32 column sums hold 32 rows before they
    go to LDS, a band reads one block row of halo for its 32, and cell rows end inside a band."""
    n, H, W, cells, band = LONG[name]
    assert band_rows(n, H, W, cells) == band and band_rows(F, 600, 64, (2, 3)) == 4
    ref, dist = long_videos(name)
    sse, q = ops.sphere_quality(dev(ref), dev(dist), cells)
    assert np.array_equal(sse.cpu().numpy(), qr.sse(ref, dist, cells))
    assert np.array_equal(q.cpu().numpy(), qr.ssim_q(ref, dist, cells))


@pytest.mark.parametrize('name', ['band32_one_band', 'band32_halo'])
def test_long_bands_black_against_white(name):
    """Every term is 65025 a_y, and a_y is 1024 around the equator: the 32 rows a u32 column sum is given come to 2^31, the most
    it ever holds (32 x 65025 x 1024 < 2^32) and more than a signed or a narrower sum would."""
    n, H, W, cells, band = LONG[name]
    assert band_rows(n, H, W, cells) == 32
    ref = torch.zeros((n, H, W, 3), dtype=torch.uint8, device='cuda')
    dist = torch.full((n, H, W, 3), 255, dtype=torch.uint8, device='cuda')
    sse, q = ops.sphere_quality(ref, dist, cells)
    cw, ww = ops.quality_cell_weights(H, W, cells), ops.quality_window_weights(H, W, cells)
    assert np.array_equal(sse.cpu().numpy(), np.broadcast_to((65025 * cw)[None, :, None], (n, cw.size, 3)))
    assert np.array_equal(q.cpu().numpy(), np.broadcast_to((26 * ww)[None, :], (n, ww.size)))


# ----------------------------------------------------------------------------- end to end
def scene():
    """K17's scene as tests/test_streaming_gpu.py builds it: a target that moves 3 degrees a frame and twelve viewers who follow
    it.  The video is a 96 x 192 texture; its four levels drop 6, 4, 2 and 0 low bits of every byte - a stand-in for a ladder of
    encodes, not an encoder."""
    n, fps = 24, 8.0
    lon = np.deg2rad(-40.0 + 3.0 * np.arange(n))
    lat = np.deg2rad(10.0 + 0.5 * np.arange(n))
    tf = (np.arange(n) + 0.5) / fps
    d = np.deg2rad(np.array([[-6, 2], [5, -3], [0, 4], [3, 3], [-4, -4], [6, 0], [-2, 5], [1, -5], [4, 2], [-5, 1], [2, -2], [0, 0]], float))
    R, off, _ = headtrack.head_cameras([(tf, lon + dx, lat + dy) for dx, dy in d], fps, n)
    rng = np.random.default_rng(2026)
    ref = rng.integers(0, 256, (n, 96, 192, 3), dtype=np.uint8)
    encodes = [(ref >> b) << b for b in (6, 4, 2, 0)]
    return n, fps, R, off, ref, encodes


def test_end_to_end_on_recorded_viewers():
    n, fps, R, off, ref, encodes = scene()
    cells, tiles = (24, 48), (6, 12)
    sq = quality.SphereQuality(cells=cells)
    seg = streaming.segment_offsets(n, fps)
    assert seg.tolist() == [0, 8, 16, 24]
    dist = sq.rd_table(ref, encodes, seg, tiles)
    want_sse = [qr.sse(ref, e, cells) for e in encodes]
    w = ops.quality_cell_weights(96, 192, tiles).astype(np.float64)
    want_dist = np.stack([np.stack([qr.coarsen(s, cells, tiles)[a:b].sum(axis=(0, 2)) for a, b in zip(seg[:-1], seg[1:])]) for s in want_sse], 2)
    assert dist.shape == (3, 72, 4) and np.array_equal(dist, want_dist / (3.0 * 8.0 * w[None, :, None]))
    assert np.all(np.diff(dist, axis=2) < 0.0) and not dist[:, :, 3].any()          # every tile has texture
    # the viewers' footprints on the cells are the demand (the share of the viewers who need the tile) and the judge
    counts, _ = ops.head_footprints(dev(np.asarray(R)), dev(np.asarray(off)), cells, (1.0, 1.0), 100.0)
    need = quality.coarsen(counts.reshape(n, -1).cpu().numpy().astype(np.int64), cells, tiles)
    demand = np.stack([need[a:b].max(axis=0) for a, b in zip(seg[:-1], seg[1:])]).astype(np.float64)
    bits = streaming._tile_cost(sq.cell_weights(cells=tiles), np.array([1.0e6, 2.0e6, 4.0e6, 8.0e6]), 1.0)
    budget = bits[:, 1].sum() * (1.0 + 1e-9)                            # the cost of the uniform plan at level 1
    levels = streaming.allocate_measured(demand, bits, dist, budget)
    spent = bits[np.arange(72)[None, :], levels].sum(axis=1)
    assert levels.shape == (3, 72) and np.all(spent <= budget) and levels.max() > 1 and levels.min() == 0
    by = torch.stack([sq.measure(ref, e, ssim=False)['sse'] for e in encodes])
    assert np.array_equal(by.cpu().numpy(), np.stack(want_sse))
    plan = sq.seen_psnr(sq.plan_sse(levels, seg, by, tiles), counts)
    flat = sq.seen_psnr(sq.plan_sse(np.ones_like(levels), seg, by, tiles), counts)
    print('seen PSNR: plan %.4f dB, uniform level 1 %.4f dB' % (float(plan.mean()), float(flat.mean())))
    assert bool((plan >= flat).all()) and float(plan.mean()) > float(flat.mean()) + 3.0
    # the restatement's numbers for this scene (tests/quality_restate.py and headtrack_restate.footprints on the CPU, whose float32
    # and float64 decisions agree on every cell here): integers exactly, the two means to the last digits of a float64 log10
    assert int(counts.sum()) == 49872 and np.bincount(levels.reshape(-1), minlength=4).tolist() == [142, 18, 55, 1]
    assert abs(float(plan.mean()) - 41.58435702192133) <= 1e-9 and abs(float(flat.mean()) - 29.243394400401524) <= 1e-9
    assert torch.equal(sq.seen_psnr(by[1].cpu(), torch.ones_like(counts).cpu()), sq.ws_psnr(by[1].cpu()))
    assert torch.allclose(sq.seen_psnr(by[1], torch.ones_like(counts)), sq.ws_psnr(by[1]), rtol=1e-14, atol=0.0)
