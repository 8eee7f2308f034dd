"""Farneback optical flow (K10) without a GPU: the library's host routines (level geometry, Gaussian taps, expansion tables),
the float64 restatement of the specification (tests/farneback_restate.py) against analytic answers - the polynomial expansion of
a quadratic image, the recovery of a known translation, which also pins the sign convention - and the refusals."""
import ctypes as C

import numpy as np
import pytest

from cp_360_weakly_supervised_saliency_amd import _lib, ops
from cp_360_weakly_supervised_saliency_amd.utils import npy_io
from cp_360_weakly_supervised_saliency_amd.utils.optical_flow import FarnebackFlow, absflow_of
from tests import farneback_restate as fb


# ----------------------------------------------------------------------------- 1. level geometry
def test_level_geometry_of_the_reference_resolution():
    geo = ops.optflow_levels(480, 960)
    assert [(h, w) for h, w, _, _ in geo] == [(480, 960), (240, 480), (120, 240), (60, 120)]          # L = 3
    assert [k for _, _, k, _ in geo] == [3, 3, 9, 19]              # cvRound(2.5) = 2, (7.5) = 8, (17.5) = 18, each | 1
    assert [s for _, _, _, s in geo] == [0.0, 0.5, 1.5, 3.5]
    assert geo == fb.level_geometry(480, 960)


@pytest.mark.parametrize('hw,want', [((64, 128), [(64, 128), (32, 64)]), ((48, 96), [(48, 96)]),
                                     ((67, 131), [(67, 131), (34, 66)])])
def test_level_geometry_small_images(hw, want):
    """64 x 128: 32 is not < 32, so one coarser level; 48 x 96: none; 67 x 131: 33.5 and 65.5 round to even."""
    geo = ops.optflow_levels(*hw)
    assert [(h, w) for h, w, _, _ in geo] == want
    assert geo == fb.level_geometry(*hw)


def test_levels_argument_caps_the_pyramid():
    assert len(ops.optflow_levels(480, 960, 0.5, 0)) == 1
    assert len(ops.optflow_levels(480, 960, 0.5, 1)) == 2
    assert len(ops.optflow_levels(480, 960, 0.5, 7)) == 4
    assert ops.optflow_levels(480, 960, 0.5, 1) == fb.level_geometry(480, 960, 0.5, 1)
    geo = ops.optflow_levels(300, 500, 0.8, 20)
    assert geo == fb.level_geometry(300, 500, 0.8, 20) and len(geo) == 11             # 300 * 0.8^10 = 32.2, * 0.8^11 = 25.8
    with pytest.raises(ValueError):
        ops.optflow_levels(480, 960, 1.0, 3)
    with pytest.raises(ValueError):
        ops.optflow_levels(0, 960)


# ----------------------------------------------------------------------------- host tables
@pytest.mark.parametrize('ksz,sigma', [(3, 0.0), (3, 0.5), (9, 1.5), (19, 3.5)])
def test_gauss_taps_equal_the_restatement(ksz, sigma):
    taps = ops.optflow_gauss_kernel(ksz, sigma)
    np.testing.assert_array_equal(taps, fb.gauss_kernel(ksz, sigma).astype(np.float32))
    assert abs(float(taps.astype(np.float64).sum()) - 1.0) < 1e-6
    if sigma == 0.0:
        assert taps.tolist() == [0.25, 0.5, 0.25]


def test_gauss_taps_refusals():
    with pytest.raises(ValueError):
        ops.optflow_gauss_kernel(4, 1.0)
    with pytest.raises(ValueError):
        ops.optflow_gauss_kernel(5, 0.0)                             # the fixed kernel exists for ksz 3 only


@pytest.mark.parametrize('n,sigma', [(5, 1.2), (7, 1.5)])
def test_poly_tables_equal_the_restatement(n, sigma):
    got = ops.optflow_poly_tables(n, sigma)
    want = fb.poly_tables(n, sigma)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b.astype(np.float32))
    assert got[0].shape == (2 * n + 1,) and got[3].shape == (4,)
    with pytest.raises(_lib.Cp360Error):
        ops.optflow_poly_tables(8, 1.5)                              # more than 15 taps: unsupported
    with pytest.raises(ValueError):
        ops.optflow_poly_tables(5, 0.0)


# ----------------------------------------------------------------------------- 2. expansion known answer
@pytest.mark.parametrize('n,sigma', [(5, 1.2), (7, 1.5)])
def test_expansion_of_a_quadratic_image_is_exact(n, sigma):
    """I = c + p x + q y + a x^2 + b y^2 + e xy: at every pixel at least n from the border the weighted least-squares fit is
    the image itself, R = [q + 2 b y + e x, p + 2 a x + e y, b, a, e].  Independent of the restatement's other stages; the
    tables stay in double here, so the answer holds to float64 rounding (|I| <= 2e3, 15 x 15 terms: 1e-9 is generous)."""
    c, p, q, a, b, e = 3.0, 0.7, -1.1, 0.05, -0.03, 0.02
    h, w = 2 * n + 9, 2 * n + 14
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing='ij')
    img = c + p * x + q * y + a * x * x + b * y * y + e * x * y
    R = fb.poly_exp(img, n, sigma, np.float64, round32=False)
    want = np.stack([q + 2 * b * y + e * x, p + 2 * a * x + e * y, np.full_like(x, b), np.full_like(x, a), np.full_like(x, e)])
    inner = (slice(None), slice(n, h - n), slice(n, w - n))
    assert np.max(np.abs(R[inner] - want[inner])) < 1e-9
    # with the tables rounded to float32, as the kernels get them, the answer moves by the tables' rounding only
    R32 = fb.poly_exp(img, n, sigma, np.float64)
    assert np.max(np.abs(R32[inner] - want[inner])) < 2e3 * 15 * 2.0 ** -23


# ----------------------------------------------------------------------------- 3. translation recovery
def texture(seed):
    rs = np.random.RandomState(seed)
    kx, ky = rs.uniform(-0.35, 0.35, 40), rs.uniform(-0.35, 0.35, 40)
    ph = rs.uniform(0, 2 * np.pi, 40)

    def f(x, y):
        return 127.5 + 18.0 * np.sum(np.sin(kx[:, None, None] * x[None] + ky[:, None, None] * y[None] + ph[:, None, None]), 0)
    return f


@pytest.mark.parametrize('hw', [(64, 128), (96, 192)])
@pytest.mark.parametrize('shift', [(1.5, -0.75), (3.25, 2.0), (-6.0, 4.5)])
def test_restatement_recovers_a_translation(hw, shift):
    """next(y + sy, x + sx) = prev(y, x) analytically -> flow = (sx, sy): mean endpoint error outside a 16 px border
    <= 0.05 px (the specification's author measured 0.006 - 0.017)."""
    h, w = hw
    sx, sy = shift
    f = texture(1234)
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing='ij')
    prev, nxt = f(x, y), f(x - sx, y - sy)
    flow = fb.farneback(np.stack([prev, nxt]))[0]
    assert flow.shape == (h, w, 2)
    epe = np.sqrt((flow[..., 0] - sx) ** 2 + (flow[..., 1] - sy) ** 2)[16:-16, 16:-16]
    print('translation %s at %s: mean EPE %.4f px, max %.4f px' % (shift, hw, epe.mean(), epe.max()))
    assert epe.mean() <= 0.05


# ----------------------------------------------------------------------------- 4. gray arithmetic, refusals, hand-off paths
def test_gray_arithmetic():
    assert np.all(fb.gray_from_rgb(np.zeros((4, 5, 3), np.uint8)) == 0.0)
    assert np.all(fb.gray_from_rgb(np.full((4, 5, 3), 255, np.uint8)) == 255.0)
    ramp = np.stack([np.arange(256), (np.arange(256) * 7) % 256, 255 - np.arange(256)], -1).astype(np.uint8)[None]
    got = fb.gray_from_rgb(ramp)
    assert got.dtype == np.float32 and got.shape == (1, 256)
    r, g, b = (ramp[0, :, i].astype(np.int64) for i in range(3))
    # the channels are reversed BEFORE cv2's BGR weights apply: the frame's channel 2 gets the 'B' weight 1868
    np.testing.assert_array_equal(got[0], (b * 1868 + g * 9617 + r * 4899 + 8192) // 16384)
    assert got[0, 10] == float((245 * 1868 + 70 * 9617 + 10 * 4899 + 8192) >> 14)
    assert np.max(np.abs(got[0] - (0.114 * b + 0.587 * g + 0.299 * r))) <= 0.51


def test_even_winsize_and_flags_are_refused():
    with pytest.raises(ValueError):
        FarnebackFlow((64, 128), winsize=14)
    with pytest.raises(ValueError):
        FarnebackFlow((64, 128), flags=256)
    with pytest.raises(ValueError):
        FarnebackFlow((64, 128), flags=4)
    z = np.zeros((2, 48, 96))
    with pytest.raises(ValueError):
        fb.farneback(z, winsize=14)
    with pytest.raises(ValueError):
        fb.farneback(z, flags=256)
    L = _lib.lib()
    one = C.c_void_p(16)
    args = lambda winsize, flags: (one, 1, 64, 128, 0.5, 7, winsize, 3, 5, 1.2, flags, one, one, 1 << 40, None)
    assert L.cp360_optflow_farneback(*args(14, 0)) == -1            # validation comes before any launch
    assert L.cp360_optflow_farneback(*args(15, 256)) == -8
    assert L.cp360_optflow_farneback(*args(35, 0)) == -8            # window wider than the kernel's LDS tile
    assert L.cp360_optflow_farneback(one, 1, 64, 128, 0.5, 7, 15, 3, 5, 1.2, 0, one, one, 16, None) == -1    # workspace too small
    assert L.cp360_optflow_blur_solve(one, one, 1, 8, 8, 4, None) == -1
    assert L.cp360_optflow_work_bytes(3, 64, 128, 0.5, 7) == 4 * (4 * 8192 + 4 * 5 * 8192 + 3 * 5 * 8192 + 3 * 2048 * 2)
    assert L.cp360_optflow_work_bytes(0, 64, 128, 0.5, 7) == 0


def test_absflow_threshold_rule():
    rs = np.random.RandomState(5)
    flow = rs.normal(0, 2, (12, 20, 2)).astype(np.float32)
    a = absflow_of(flow)
    assert a.dtype == np.float32 and a.min() == 0.0 and a.max() == 1.0
    mag = np.sqrt(flow[..., 0] ** 2 + flow[..., 1] ** 2)
    n = (mag - mag.min()) / (mag - mag.min()).max()
    cut = n.mean() - 1.5 * n.std()
    np.testing.assert_array_equal(a, np.where(n < cut, 0, n))
    np.testing.assert_array_equal(a, fb.absflow(flow))


def test_save_motions_index_rule(tmp_path):
    """The flow from frame i to i + 1 goes under i + 2, the number of frame i's cube_feat."""
    flows = np.arange(3 * 4 * 6 * 2, dtype=np.float64).reshape(3, 4, 6, 2)
    vd = str(tmp_path / 'vid')
    npy_io.save_motions(vd, flows)
    for t in range(3):
        assert npy_io.motion_path(vd, t + 2).endswith('motion/%06d.npy' % (t + 2))
        got = np.load(npy_io.motion_path(vd, t + 2))
        assert got.dtype == np.float32 and got.shape == (4, 6, 2)
        np.testing.assert_array_equal(got, flows[t].astype(np.float32))
    npy_io.save_motions(vd, flows[:1], first_frame_no=7)
    assert np.load(npy_io.motion_path(vd, 7)).shape == (4, 6, 2)
    with pytest.raises(ValueError):
        npy_io.save_motions(vd, flows[0])
