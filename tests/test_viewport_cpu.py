"""The viewport pilot (K12) without a GPU: the library's exports and status codes, the Python wrappers' refusals, the claims of
the float64 restatement (tests/viewport_restate.py) that tests/test_viewport_gpu.py holds the kernels to, and the parity of the
package's host code (utils/viewport.py: look_at, smooth_path) with the restatement's."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from cp_360_weakly_supervised_saliency_amd import _lib, ops
from cp_360_weakly_supervised_saliency_amd.utils import hashrng
from cp_360_weakly_supervised_saliency_amd.utils import viewport as vp
from tests import viewport_restate as vr

K12 = ('cp360_view_render', 'cp360_view_outline', 'cp360_view_smooth', 'cp360_view_peak')
NULL, BAD_SHAPE, ALIGN, UNSUPPORTED = -5, -1, -6, -8


# ----------------------------------------------------------------------------- library
def test_library_exports_the_four_symbols_at_version_306():
    L = _lib.lib()
    assert L.cp360_version() == 306 == _lib.ABI_VERSION
    for name in K12:
        assert name in _lib.PUBLIC_SYMBOLS and hasattr(L, name)


def test_status_codes_without_gpu():
    """Argument validation happens before any launch: the dummy pointers are never used."""
    L = _lib.lib()
    one, two, big = C.c_void_p(16), C.c_void_p(32), 1 << 20
    hf = math.radians(90.0)
    render = lambda dt, fr, R, N, H, W, Cn, hfov, out, h, w: L.cp360_view_render(dt, fr, R, N, H, W, Cn, hfov, out, h, w, None)
    assert render(_lib.F32, None, one, 1, 16, 32, 3, hf, two, 9, 16) == NULL
    assert render(_lib.F32, one, None, 1, 16, 32, 3, hf, two, 9, 16) == NULL
    assert render(_lib.F32, one, one, 1, 16, 32, 3, hf, None, 9, 16) == NULL
    for N, h, w in ((0, 9, 16), (1, 0, 16), (1, 9, 0), (-1, 9, 16), (1, -9, 16)):
        assert render(_lib.F32, one, one, N, 16, 32, 3, hf, two, h, w) == BAD_SHAPE
    assert render(_lib.F32, one, one, 1, 0, 32, 3, hf, two, 9, 16) == BAD_SHAPE
    for bad in (0.0, -1.0, math.pi, 4.0, float('nan')):
        assert render(_lib.F32, one, one, 1, 16, 32, 3, bad, two, 9, 16) == BAD_SHAPE
    assert render(_lib.F32, one, one, 1, 16, 32, 0, hf, two, 9, 16) == BAD_SHAPE
    assert render(_lib.F32, one, one, 1, 16, 32, 5, hf, two, 9, 16) == UNSUPPORTED
    assert render(_lib.U8, one, one, 1, 16, 32, 4, hf, two, 9, 16) == UNSUPPORTED
    assert render(_lib.F32, one, one, 70000, 16, 32, 3, hf, two, 9, 16) == UNSUPPORTED      # grid z
    assert render(_lib.F32, one, one, 1, 16, 32, 3, hf, two, 70000, 16) == UNSUPPORTED      # grid y
    assert render(_lib.F32, one, one, 1, 16, 32, 3, hf, one, 9, 16) == UNSUPPORTED          # in place
    assert render(_lib.BF16, one, one, 1, 16, 32, 3, hf, two, 9, 16) == -4

    rgb = (C.c_ubyte * 3)(0, 255, 0)
    prgb = C.cast(rgb, C.c_void_p)
    tab = L.cp360_stab_work_bytes(0, 16, 32)
    outline = lambda fr, R, N, H, W, hfov, h, w, bpx, col, out, work, nb: L.cp360_view_outline(fr, R, N, H, W, hfov, h, w, bpx, col,
                                                                                               out, work, nb, None)
    assert outline(None, one, 1, 16, 32, hf, 9, 16, 3.0, prgb, one, one, big) == NULL
    assert outline(one, None, 1, 16, 32, hf, 9, 16, 3.0, prgb, one, one, big) == NULL
    assert outline(one, one, 1, 16, 32, hf, 9, 16, 3.0, None, one, one, big) == NULL
    assert outline(one, one, 1, 16, 32, hf, 9, 16, 3.0, prgb, None, one, big) == NULL
    assert outline(one, one, 1, 16, 32, hf, 9, 16, 3.0, prgb, one, None, big) == NULL
    for N, h, w in ((0, 9, 16), (1, 0, 16), (1, 9, 0)):
        assert outline(one, one, N, 16, 32, hf, h, w, 3.0, prgb, one, one, big) == BAD_SHAPE
    assert outline(one, one, 1, 16, 32, math.pi, 9, 16, 3.0, prgb, one, one, big) == BAD_SHAPE
    assert outline(one, one, 1, 16, 32, 0.0, 9, 16, 3.0, prgb, one, one, big) == BAD_SHAPE
    assert outline(one, one, 1, 16, 32, hf, 9, 16, 0.0, prgb, one, one, big) == BAD_SHAPE
    assert outline(one, one, 1, 16, 32, hf, 9, 16, 3.0, prgb, one, one, tab - 1) == BAD_SHAPE     # workspace too small
    assert outline(one, one, 1, 16, 32, hf, 9, 16, 3.0, prgb, one, C.c_void_p(8), big) == ALIGN
    assert outline(one, one, 70000, 16, 32, hf, 9, 16, 3.0, prgb, one, one, big) == UNSUPPORTED

    sg = math.radians(15.0)
    tabm = L.cp360_stab_work_bytes(0, 14, 28)
    smooth = lambda m, F, hm, wm, s, out, work, nb: L.cp360_view_smooth(m, F, hm, wm, s, out, work, nb, None)
    assert smooth(None, 1, 14, 28, sg, two, one, big) == NULL
    assert smooth(one, 1, 14, 28, sg, None, one, big) == NULL
    assert smooth(one, 1, 14, 28, sg, two, None, big) == NULL
    for F, hm, wm in ((0, 14, 28), (1, 0, 28), (1, 14, -1)):
        assert smooth(one, F, hm, wm, sg, two, one, big) == BAD_SHAPE
    for bad in (0.0, -0.1, float('nan'), float('inf')):
        assert smooth(one, 1, 14, 28, bad, two, one, big) == BAD_SHAPE
    assert smooth(one, 1, 14, 28, sg, two, one, tabm - 1) == BAD_SHAPE
    assert smooth(one, 1, 14, 28, sg, two, C.c_void_p(8), big) == ALIGN
    assert smooth(one, 1, 128, 129, sg, two, one, big) == UNSUPPORTED                                # P > 16384
    assert smooth(one, 1, 14, 28, sg, one, one, big) == UNSUPPORTED                                  # in place

    peak = lambda sm, m, F, hm, wm, s, d, i, v, work, nb: L.cp360_view_peak(sm, m, F, hm, wm, s, d, i, v, work, nb, None)
    ok = (one, one, 1, 14, 28, sg, one, one, one, one, big)
    for k in (0, 1, 6, 7, 8, 9):
        args = list(ok)
        args[k] = None
        assert peak(*args) == NULL
    for F, hm, wm in ((0, 14, 28), (1, 0, 28), (1, 14, 0)):
        assert peak(one, one, F, hm, wm, sg, one, one, one, one, big) == BAD_SHAPE
    assert peak(one, one, 1, 14, 28, 0.0, one, one, one, one, big) == BAD_SHAPE
    assert peak(one, one, 1, 14, 28, sg, one, one, one, one, tabm - 1) == BAD_SHAPE
    assert peak(one, one, 1, 14, 28, sg, one, one, one, C.c_void_p(8), big) == ALIGN
    assert peak(one, one, 1, 129, 128, sg, one, one, one, one, big) == UNSUPPORTED


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    frames = torch.zeros(1, 16, 32, 3, dtype=torch.uint8)
    R = torch.eye(3)[None]
    maps = torch.zeros(1, 14, 28)
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.viewport_render(frames, R, (9, 16), 90.0)
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.viewport_outline(frames, R, (9, 16), 90.0)
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.sphere_smooth(maps)
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.sphere_peak(maps)
    with pytest.raises(ValueError):
        vp.ViewportPilot((36, 64), hfov_deg=180.0, device='cpu')
    with pytest.raises(ValueError):
        vp.ViewportPilot((36, 64), sigma_deg=0.0, device='cpu')
    with pytest.raises(ValueError):
        vp.smooth_path(np.zeros((3, 2)))
    with pytest.raises(ValueError):
        ops._view_geometry((9, 16), 0.0)
    with pytest.raises(ValueError):
        ops._view_geometry((0, 16), 90.0)
    with pytest.raises(ValueError):
        ops._view_maps(torch.zeros(1, 14, 28), -1.0)
    with pytest.raises(ValueError):
        ops._view_maps(torch.zeros(1, 129, 128), 15.0)
    with pytest.raises(ValueError):
        ops._view_maps(torch.zeros(14, 28), 15.0)


# ----------------------------------------------------------------------------- the restatement's own claims
@pytest.mark.parametrize('hw', [(9, 17), (17, 31)])
@pytest.mark.parametrize('HW', [(16, 32), (33, 66)])
def test_identity_camera_looks_at_the_panorama_centre(hw, HW):
    H, W = HW
    sx, sy = vr.sample_positions(np.eye(3), hw, 70.0, H, W)
    assert abs(sx[hw[0] // 2, hw[1] // 2] - (W / 2 - 0.5)) < 1e-12
    assert abs(sy[hw[0] // 2, hw[1] // 2] - (H / 2 - 0.5)) < 1e-12
    # right of the view is right on the panorama, up is up
    assert sx[hw[0] // 2, -1] > sx[hw[0] // 2, 0] and sy[0, hw[1] // 2] < sy[-1, hw[1] // 2]
    # the view's edge is hfov / 2 away from its centre: the first column's outer edge lies half a view pixel further out
    f, up, rt = vr.view_rays(hw, 70.0)
    tx = math.tan(math.radians(35.0))
    assert abs(rt[hw[0] // 2, 0] / f[hw[0] // 2, 0] + tx * (1 - 1 / hw[1])) < 1e-12


def test_render_of_a_constant_image_is_constant():
    frames = np.full((2, 16, 32, 3), 0.625)
    R = np.stack([vr.rot((0.3, 0.8, -0.52), 1.1), vr.rot((1, 0, 0), 0.5 * np.pi)])
    assert np.all(vr.render(frames, R, (9, 16), 100.0) == 0.625)
    assert np.all(vr.render(frames.astype(np.float32), R, (9, 16), 100.0, np.float32) == np.float32(0.625))
    u8 = np.full((1, 16, 32, 3), 77, np.uint8)
    assert np.all(vr.render(u8, R[:1], (9, 16), 100.0) == 77)


def test_look_at():
    assert np.array_equal(vr.look_at((1.0, 0.0, 0.0)), np.eye(3))
    assert np.array_equal(vp.look_at((1.0, 0.0, 0.0)), np.eye(3))
    dirs = hashrng.normal(900, (20, 3), dtype=np.float64)
    for d in dirs:
        R = vr.look_at(d)
        assert np.max(np.abs(R.T @ R - np.eye(3))) < 1e-14 and abs(np.linalg.det(R) - 1.0) < 1e-14
        assert np.max(np.abs(R[:, 0] - d / np.linalg.norm(d))) < 1e-15
        assert abs(R[1, 2]) < 1e-15 and R[1, 1] > 0                  # a level horizon: right has no y, up points up
    # a path over the pole keeps its right: no flip on the way, the pole itself takes the previous frame's
    prev = vr.look_at((math.cos(1.5), math.sin(1.5), 0.0))[:, 2]
    at = vr.look_at((0.0, 1.0, 0.0), prev)
    assert np.max(np.abs(at[:, 2] - prev)) < 1e-12
    assert np.max(np.abs(at.T @ at - np.eye(3))) < 1e-14 and abs(np.linalg.det(at) - 1.0) < 1e-14
    first = vr.look_at((0.0, -1.0, 0.0))
    assert np.array_equal(first[:, 2], (0.0, 0.0, 1.0)) and abs(np.linalg.det(first) - 1.0) < 1e-14


def test_smooth_path():
    c0 = np.array([0.6, 0.0, 0.8])
    const = vr.smooth_path(np.stack([c0] * 7))
    assert np.max(np.abs(const - c0)) < 1e-15
    # a noisy pan: unit vectors, and the step limit holds between consecutive outputs
    t = np.linspace(0.0, 2.5, 30)
    c = np.stack([np.cos(t), 0.3 * np.sin(3 * t), np.sin(t)], 1) + 0.2 * hashrng.normal(901, (30, 3), dtype=np.float64)
    for max_step in (None, 2.0):
        m = vr.smooth_path(c, 0.7, max_step)
        assert np.max(np.abs(np.linalg.norm(m, axis=1) - 1.0)) < 1e-15
        if max_step is not None:
            steps = [vr.angle(m[i], m[i + 1]) for i in range(29)]
            assert max(steps) <= np.deg2rad(max_step) + 1e-12
            assert max(vr.angle(a, b) for a, b in zip(c[:-1], c[1:])) > np.deg2rad(4 * max_step)
    # alpha = 0 follows the targets
    assert np.max(np.abs(vr.smooth_path(c, 0.0) - c / np.linalg.norm(c, axis=1, keepdims=True))) < 1e-12
    # antipodal jumps, also along the fallback axis
    for a in ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, -1.0)):
        a = np.array(a)
        m = vr.smooth_path(np.stack([a, -a, -a, a]), 0.5)
        assert np.all(np.isfinite(m)) and np.max(np.abs(np.linalg.norm(m, axis=1) - 1.0)) < 1e-15
        assert vr.angle(m[0], m[2]) > 0.1                             # it did move


def test_host_code_parity():
    t = np.linspace(0.0, 4.0, 25)
    c = np.stack([np.cos(t) * np.cos(0.4 * t), np.sin(0.4 * t), np.sin(t) * np.cos(0.4 * t)], 1)
    c = c + 0.1 * hashrng.normal(902, c.shape, dtype=np.float64)
    c[7] = -c[6]                                                       # an antipodal jump
    c[15] = (0.0, 1.0, 0.0)                                            # a pole
    for alpha, ms in ((0.85, None), (0.5, 3.0), (0.0, 10.0)):
        got, want = vp.smooth_path(c, alpha, ms), vr.smooth_path(c, alpha, ms)
        assert np.max(np.abs(got - want)) < 1e-12
    assert np.max(np.abs(vp.cameras(c) - vr.cameras(c))) < 1e-12
    prev = (0.0, 0.6, 0.8)
    for d in ((0.0, 1.0, 0.0), (0.0, -1.0, 1e-9), (0.2, -0.3, 0.5)):
        assert np.max(np.abs(vp.look_at(d, prev) - vr.look_at(d, prev))) < 1e-12


@pytest.mark.parametrize('hw', [(5, 9), (14, 28)])
def test_smooth_keeps_a_constant_map(hw):
    for dtype in (np.float64, np.float32):
        out = vr.smooth(np.full((1,) + hw, 0.375), 15.0, dtype)
        assert np.max(np.abs(out - 0.375)) < (1e-12 if dtype is np.float64 else 1e-6)


def test_peak_of_a_blob_between_pixel_centres():
    """One vMF blob whose centre lies between pixel centres of a 14 x 28 map: the mean-shift step lands within 0.1 map pixel
    of it, the argmax alone up to 0.71 pixel away.

    The widths.  The step's window (sigma_k, centred on the argmax p*) multiplies the blob (sigma_b, centred on c0): the product of
    the two Gaussians has its mean at (c0 / sigma_b^2 + p* / sigma_k^2) / (1 / sigma_b^2 + 1 / sigma_k^2), so one step leaves
    the fraction sigma_b^2 / (sigma_b^2 + sigma_k^2) of the argmax's offset - half of it when the window is as wide as the
    blob.  0.1 pixel of at most sqrt(1/2) pixel needs a fraction of 0.14 at most, sigma_k >= 2.5 sigma_b; a blob the 12.9-degree
    grid still samples has sigma_b of 6 degrees or more.  Hence sigma_b = 8 and sigma_k = 30 degrees: the fraction is 0.066, 0.047
    pixel in the worst position, which leaves half of the bound to the grid's discretisation."""
    hm, wm = 14, 28
    for x, y in ((9.5, 4.5), (20.3, 8.6), (27.5, 6.5), (3.4, 2.5), (13.5, 0.5), (5.0, 6.5)):
        from tests.stabilize_restate import dir_
        centre = dir_(x, y, hm, wm)
        maps = vr.vmf_blob(centre, hm, wm, 8.0)[None]
        dirs, idx, val = vr.peak(maps, 30.0)
        got = vr.map_position(dirs[0], hm, wm)
        ex = (got[0] - x + wm / 2) % wm - wm / 2
        err = math.hypot(ex, got[1] - y)
        assert err < 0.1, (x, y, got, err)
        assert vr.angle(dirs[0], centre) < 0.1 * 2 * np.pi / wm


def test_peak_edge_cases():
    maps = np.full((2, 5, 9), np.nan)
    maps[1] = 0.0
    maps[1, 2, 3] = maps[1, 2, 7] = 1.0
    dirs, idx, val = vr.peak(maps, 8.0)
    assert idx[0] == -1 and np.array_equal(dirs[0], (1.0, 0.0, 0.0)) and np.isnan(val[0])
    assert idx[1] in (2 * 9 + 3, 2 * 9 + 7)
    # an exact tie (the smoothed values of two pixels differ in their last bits: the map itself stands in) takes the lowest index
    dirs, idx, val = vr.peak(maps[1:], 8.0, smoothed=maps[1:])
    assert idx[0] == 2 * 9 + 3 and val[0] == 1.0
    assert vr.argmax_finite([np.nan, 2.0, np.inf, 2.0]) == 1 and vr.argmax_finite([np.nan, np.inf]) == -1


@pytest.mark.parametrize('border_px', [1, 3])
def test_outline_mask_is_symmetric(border_px):
    H, W = 64, 128
    mask, u, v, df, thr = vr.outline(np.eye(3), H, W, (36, 64), 90.0, border_px)
    assert mask.any() and not mask.all()
    assert np.array_equal(mask, mask[:, ::-1]) and np.array_equal(mask, mask[::-1, :])
    # a frame: the view's centre is not marked, nor is anything behind the camera
    assert not mask[H // 2, W // 2] and not mask[:, :W // 4].any() and not mask[:, -(W // 4):].any()
    assert not vr.outline(np.full((3, 3), np.nan), H, W, (36, 64), 90.0, border_px)[0].any()
    bad = np.eye(3)
    bad[0, 0] = np.inf
    assert not vr.outline(bad, H, W, (36, 64), 90.0, border_px)[0].any()
