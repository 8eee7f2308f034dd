"""The conditions tests/test_sphere_paths_gpu.py rests on, without a GPU: the walk's geometry and the share of the pairs float32
cannot decide on the wide grids, the overlap of the zoom cameras with their viewers, the launch geometry of the default grid, of
3072 tiles and of the source limit, the conditioning of the 65 ego-motion fits, the seam crossing of the wide flows, the 65
sequences whose trace is not their frames' argmax, and the blocks the zoom outlines' borders lie in."""
import numpy as np
import pytest

from tests import headtrack_restate as hr
from tests import test_sphere_paths_gpu as sp


@pytest.mark.parametrize('name', sorted(sp.WIDE_HEAD))
def test_wide_head_cases(name):
    c = sp.head_case(name)
    (h, w), N = c['grid'], len(c['R'])
    assert c['offsets'].tolist() == ([0, 3, 3, 8, 73] if h == 120 else [0, 4, 5, 5, 7]) and N == c['offsets'][-1]
    wraps = np.arange(w) + 64 >= w                                     # a step of 64 from column x
    assert not (np.arange(64) // w).any() and wraps.any() and not wraps.all() and not (np.arange(w) + 64 >= 2 * w).any()
    # the camera's windows meet some of their viewers' and miss others: inter is neither 0 nor uni throughout
    b = hr.agreement_bounds(c)
    assert (b[0] > 0).any() and (b[1] == 0).any() and (b[1] < b[2]).all()
    zb = sp.zoom_bounds_case(name)
    assert zb['cins'].shape == (4, h, w) and zb['cins'].reshape(4, -1).any(1).all()


@pytest.mark.parametrize('name', sorted(sp.WIDE_QUALITY))
def test_wide_quality_cases(name):
    c, L = sp.quality_case(name)
    assert c['grid'][1] > 64 and 1 <= L <= 8 and c['a_grid'].shape == (c['grid'][0],)


@pytest.mark.parametrize('src', sorted(sp.DEFAULT_SOURCES))
def test_default_grid_cases(src):
    c = sp.default_grid_case(src)
    assert c['ins'].shape == (src[0] * src[1], 28800) and c['ins'][:, 256 * 32:].any()      # pairs inside in the later blocks' words


def test_tile_and_limit_cases():
    c = sp.tile_case()
    assert c['tiles'] == c['grid'] == (48, 64) and c['ins'][:, 2048:].any()                  # tiles of the second block are lit
    c = sp.limit_case()
    assert c['ins'].shape == (4096, 288) and c['ins'][3840:].any() and c['a_src'].shape == (64,)


def test_ego_cases():
    flow, want, d32 = sp.fit65_case()
    assert flow.shape == (65, 16, 32, 2) and want[0].shape == (65, 3, 3) and float(np.max(d32[1])) < 1e-5
    assert len({float(np.abs(f).sum()) for f in flow}) == 65           # 65 different flows
    for hw in sp.WIDE_FLOWS:
        assert sp.residual_blocks(hw) == (hw[1] + 255) // 256 > 1


def test_path_case():
    s, g, starts, idx, score = sp.path65_case()
    assert s.shape == (70, 5, 9) and len(starts) == 66 and score.shape == (65,) and np.diff(starts).tolist().count(1) == 61
    assert int(starts[64]) == 67 and int(starts[65]) == 70             # sequence 64: frames 67 .. 69


@pytest.mark.parametrize('HW,border_px,blocks', [((9, 300), 1, [[0], [0], [0, 1], [0]]), ((9, 300), 3, [[0], [0, 1], [0, 1], [0]]),
                                                 ((12, 520), 1, [[0, 1], [0, 1], [0, 1], [0]]),
                                                 ((12, 520), 3, [[0, 1], [0, 1], [0, 1], [0]])])
def test_zoom_outline_blocks(HW, border_px, blocks):
    assert sp.zoom_outline_blocks(HW, border_px) == blocks
