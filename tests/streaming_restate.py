"""Numpy restatement of viewport-adaptive streaming (K24, csrc/streaming.hip and utils/streaming.py; the specification is
DESIGN.md "K24").  A source map has hs x ws pixels; pixel j stands for a viewer whose head points at its centre, the level camera
cam_j = look_at(dir(x_j, y_j)), float64 rounded once to float32.  The window is K17's view ((h_v, w_v), hfov_deg).

    incidence   inc[j, i] = inside(cam_j, dir(i)) on the h x w grid, tests/headtrack_restate.py's decision; as bits, pixel i is bit
                i % 32 of u32 word i / 32, the bits past P = h w are 0
    mass        m[f, j] = sal[f, j] float(a_y(row of j)) if sal[f, j] > 0 and finite, else 0
    expect      acc = 0; for j ascending: if inc[j, i]: acc = acc + m[f, j]; total[f] the same over every j;
                out[f, i] = total > 0 ? acc / total : 0 - in float32, in this order (``expect32``), or in float64 (``expect64``)
    tiles       pixel (x, y) in tile ((y rows) / h) cols + (x cols) / w; tinc[j, t] = OR of inc[j, i] over the tile;
                area[t] = sum of a_y over the tile's pixels
    qarea       qarea[k, l] = sum a_y [inside(R_k, dir(i)) and min(levels[f_k, tile(i)], L - 1) == l]

The (camera, pixel) pairs that float32 cannot decide are ``headtrack_restate.classify``'s: |u| or |v| within 8 d32 of its
threshold.  Nothing here imports the code under test but the host table of the row weights.
"""
import functools

import numpy as np

from tests import headtrack_restate as hr
from tests import viewport_restate as vr


def cameras(src_hw):
    """float32 [hs ws, 3, 3]: look_at of every pixel centre's direction, in float64, rounded once."""
    hs, ws = src_hw
    out = np.empty((hs * ws, 3, 3), np.float64)
    for y in range(hs):
        phi = (1.0 - 2.0 * (y + 0.5) / hs) * np.pi / 2.0
        for x in range(ws):
            theta = (2.0 * (x + 0.5) / ws - 1.0) * np.pi
            out[y * ws + x] = vr.look_at([np.cos(phi) * np.cos(theta), np.sin(phi), np.cos(phi) * np.sin(theta)])
    return out.astype(np.float32)


def pixel_dirs(hw):
    """float64 [h w, 3]: dir of every pixel centre."""
    h, w = hw
    phi = ((1.0 - 2.0 * (np.arange(h) + 0.5) / h) * np.pi / 2.0)[:, None]
    theta = ((2.0 * (np.arange(w) + 0.5) / w - 1.0) * np.pi)[None, :]
    return np.stack([np.cos(phi) * np.cos(theta), np.sin(phi) * np.ones_like(theta), np.cos(phi) * np.sin(theta)], -1).reshape(-1, 3)


def pack_bits(b):
    """bool [S, P] -> uint32 [S, ceil(P / 32)]: element i is bit i % 32 of word i / 32."""
    S, P = b.shape
    pad = np.zeros((S, (P + 31) // 32 * 32), np.uint64)
    pad[:, :P] = b
    return (pad.reshape(S, -1, 32) << np.arange(32, dtype=np.uint64)[None, None, :]).sum(axis=2).astype(np.uint32)


def unpack_bits(words, P):
    """uint32 [S, W] -> bool [S, P]."""
    words = np.asarray(words).view(np.uint32) if np.asarray(words).dtype == np.int32 else np.asarray(words, np.uint32)
    b = (words[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :]) & np.uint32(1)
    return b.reshape(words.shape[0], -1)[:, :P].astype(bool)


def tile_index(hw, tiles):
    """int64 [h w]: the tile of every pixel."""
    (h, w), (rows, cols) = hw, tiles
    return ((((np.arange(h) * rows) // h) * cols)[:, None] + ((np.arange(w) * cols) // w)[None, :]).reshape(-1)


def tile_or(inc, hw, tiles):
    """bool [S, P] -> bool [S, T]."""
    idx, T = tile_index(hw, tiles), tiles[0] * tiles[1]
    out = np.zeros((inc.shape[0], T), bool)
    for t in range(T):
        out[:, t] = inc[:, idx == t].any(axis=1)
    return out


def tile_area(hw, tiles, weights):
    """int64 [T]: the sum of a_y over the tile's pixels."""
    a, idx = np.repeat(np.asarray(weights, np.int64), hw[1]), tile_index(hw, tiles)
    return np.array([int(a[idx == t].sum()) for t in range(tiles[0] * tiles[1])], np.int64)


def mass(sal, weights, dtype=np.float32):
    """sal [F, hs, ws], weights int [hs] -> m dtype [F, hs ws]: one multiplication in dtype."""
    sal = np.asarray(sal, np.float32)
    F, hs, ws = sal.shape
    a = np.asarray(weights, np.int64).astype(dtype)[None, :, None]
    with np.errstate(invalid='ignore', over='ignore'):
        keep = (sal > 0) & np.isfinite(sal)
        m = np.where(keep, sal.astype(dtype) * a, dtype(0))
    return m.reshape(F, hs * ws).astype(dtype)


def expect32(sal, weights, bits):
    """The definition in float32, in its order; bits bool [S, P] -> (out float32 [F, P], total float32 [F])."""
    m = mass(sal, weights, np.float32)
    F, S = m.shape
    acc, tot = np.zeros((F, bits.shape[1]), np.float32), np.zeros(F, np.float32)
    with np.errstate(over='ignore', invalid='ignore'):
        for j in range(S):
            acc = np.where(bits[j][None, :], acc + m[:, j, None], acc).astype(np.float32)
            tot = (tot + m[:, j]).astype(np.float32)
        out = np.where(tot[:, None] > 0, acc / np.where(tot > 0, tot, np.float32(1))[:, None], np.float32(0)).astype(np.float32)
    return out, tot


def expect64(sal, weights, bits):
    """The same quantity in float64 -> (out float64 [F, P], total float64 [F])."""
    m = mass(sal, weights, np.float64)
    tot = m.sum(axis=1)
    acc = m @ bits.astype(np.float64)
    return np.where(tot[:, None] > 0, acc / np.where(tot > 0, tot, 1.0)[:, None], 0.0), tot


def qarea(masks, offsets, hw, tiles, weights, levels, L):
    """masks bool [N, h, w] of the viewers, levels int [F, T] -> int64 [N, L]."""
    N = len(masks)
    idx = tile_index(hw, tiles)
    a = np.repeat(np.asarray(weights, np.int64), hw[1])
    fr = hr.frame_of(offsets, N)
    out = np.zeros((N, L), np.int64)
    for k in range(N):
        lv = np.minimum(np.asarray(levels, np.int64)[fr[k]], L - 1)[idx]
        for l in range(L):
            out[k, l] = int(a[masks[k].reshape(-1) & (lv == l)].sum())
    return out


def window_solid_angle(view):
    """4 asin(tx ty / sqrt((1 + tx^2)(1 + ty^2))), the solid angle of a rectangular window."""
    tx, ty = (float(v) for v in hr.tangents(view))
    return 4.0 * np.arcsin(tx * ty / np.sqrt((1.0 + tx * tx) * (1.0 + ty * ty)))


# ----------------------------------------------------------------------------- test inputs shared by the CPU and GPU tests
SQ100 = ((1, 1), 100.0)
# name -> (source, grid, window, tiles, weights)
CASES = {
    's2x4_g5x9': ((2, 4), (5, 9), SQ100, (2, 3), 'solid_angle'),
    's4x8_g12x24': ((4, 8), (12, 24), SQ100, (3, 4), 'solid_angle'),
    's4x8_g12x24_wide': ((4, 8), (12, 24), ((1, 1), 170.0), (1, 1), 'uniform'),
    's4x8_g12x24_narrow': ((4, 8), (12, 24), ((1, 1), 10.0), (3, 4), 'solid_angle'),
    's7x14_g12x24': ((7, 14), (12, 24), SQ100, (3, 4), 'solid_angle'),
    's7x14_g30x60': ((7, 14), (30, 60), SQ100, (6, 12), 'solid_angle'),
    's7x14_g30x60_9x16': ((7, 14), (30, 60), ((9, 16), 75.0), (6, 12), 'uniform'),
    's4x8_g30x60_3x4': ((4, 8), (30, 60), ((3, 4), 100.0), (6, 12), 'solid_angle'),
    's14x28_g30x60': ((14, 28), (30, 60), SQ100, (6, 12), 'solid_angle'),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict: src, grid, view, tiles, mode, cams float32 [S, 3, 3], the float64 classification of the gaze cameras on the grid
    (ins, und bool [S, P]), the row weights of the source map (a_src) and of the grid (a_grid)."""
    return make_case(name, *CASES[name])


def make_case(name, src, grid, view, tiles, mode):
    """``case`` for inputs that are not in CASES (tests/test_sphere_paths_gpu.py builds the large grids and sources with it)."""
    cams = cameras(src)
    ins, und = hr.classify(cams, grid[0], grid[1], view)
    S = src[0] * src[1]
    return dict(name=name, src=src, grid=grid, view=view, tiles=tiles, mode=mode, cams=cams, ins=ins.reshape(S, -1),
                und=und.reshape(S, -1), a_src=hr.row_weights(src[0], mode), a_grid=hr.row_weights(grid[0], mode))


def random_maps(seed, F, src):
    """Positive float32 maps [F, hs, ws] with a wide range of values."""
    from cp_360_weakly_supervised_saliency_amd.utils import hashrng
    return np.exp(2.0 * hashrng.normal(seed, (F,) + tuple(src), dtype=np.float64)).astype(np.float32)
