"""The specification of the 360-degree stabilisation (K11, DESIGN.md "K11") on the CPU: the claims of its float64 restatement
(tests/stabilize_restate.py) that the GPU tests then rest on - the fit recovers a rotation from its own flow, the graduated
Geman-McClure weights reject a moving rectangle that plain least squares follows, the resampler is continuous over the seam
and the poles - and the argument checks of the C entry points, which need no GPU."""
import ctypes as C

import numpy as np
import pytest

from cp_360_weakly_supervised_saliency_amd import _lib
from tests import stabilize_restate as sr

SIZES = [(32, 64), (120, 240)]
ANGLES = [0.5, 3.0, 10.0]


@pytest.mark.parametrize('hw', SIZES)
@pytest.mark.parametrize('deg', ANGLES)
def test_fit_recovers_a_rotation_from_its_own_flow(hw, deg):
    """Clean flow rotation_flow(R_true) about a non-axis direction: R = R_true elementwise to 1e-9 after 3 iterations."""
    R_true = sr.rot(sr.AXIS, np.deg2rad(deg))
    R, diag = sr.rotation_fit(sr.rotation_flow(R_true, *hw), iters=3)
    err = float(np.max(np.abs(R - R_true)))
    print('clean %s %.1f deg: max|R - R_true| = %.2e, RMS residual %.2e px' % (hw, deg, err, diag[2]))
    assert err <= 1e-9


@pytest.mark.parametrize('hw', SIZES)
@pytest.mark.parametrize('deg', ANGLES)
def test_robust_fit_rejects_a_moving_rectangle(hw, deg):
    """Flow + 0.05 px noise + a rectangle of 45 % x 45 % of the image shifted by (3, -1.5) px: the robust fit's angular error is at
    most 1 / 20 of plain least squares' (iters = 1) on the same input.  Measured here: 375 to 3300 times smaller
    (least squares 1.18 - 1.23 px-equivalents, robust 0.0004 - 0.003)."""
    H, W = hw
    R_true = sr.rot(sr.AXIS, np.deg2rad(deg))
    flow = sr.noisy_outlier_flow(R_true, H, W, 100 + int(10 * deg))
    ys, xs = sr.outlier_box(H, W)
    assert 0.19 <= (ys.stop - ys.start) * (xs.stop - xs.start) / float(H * W) <= 0.21
    e_ls = sr.angle_between(sr.rotation_fit(flow, iters=1)[0], R_true)
    e_rb = sr.angle_between(sr.rotation_fit(flow)[0], R_true)
    print('robust %s %.1f deg: least squares %.4f px, robust %.5f px, ratio %.0f' % (hw, deg, e_ls * W / (2 * np.pi),
                                                                                   e_rb * W / (2 * np.pi), e_ls / e_rb))
    assert e_rb <= e_ls / 20.0


@pytest.mark.parametrize('hw', SIZES + [(33, 66)])
def test_flow_of_the_identity_is_zero(hw):
    """pix(dir(x, y)) = (x, y) up to float64's rounding, which asin amplifies by 1 / cos phi in the rows next to a pole."""
    H, W = hw
    G = sr.rotation_flow(np.eye(3), H, W)
    assert G.shape == (H, W, 2)
    assert float(np.max(np.abs(G))) <= 64 * np.finfo(np.float64).eps * max(H, W) / np.sin(np.pi / (2 * H))


@pytest.mark.parametrize('hw', SIZES)
def test_fit_of_the_inverse_flow_composes_to_the_identity(hw):
    R_true = sr.rot(sr.AXIS, np.deg2rad(3.0))
    Ra = sr.rotation_fit(sr.rotation_flow(R_true, *hw), iters=3)[0]
    Rb = sr.rotation_fit(sr.rotation_flow(R_true.T, *hw), iters=3)[0]
    assert float(np.max(np.abs(Rb @ Ra - np.eye(3)))) <= 1e-9


def test_geometry_follows_sph_utils():
    """dir is to_3dsphere(xy2angle(..)) of utils/sph_utils.py, pix inverts it, and it continues smoothly over a pole."""
    from cp_360_weakly_supervised_saliency_amd.utils import sph_utils
    H, W = 12, 20
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    th, ph = sph_utils.xy2angle(x, y, W, H)
    want = np.stack(sph_utils.to_3dsphere(th, ph, 1.0), -1)
    np.testing.assert_allclose(sr.dir_(x, y, H, W), want, atol=1e-15)
    sx, sy = sr.pix(want, H, W)
    np.testing.assert_allclose(sx, x, atol=1e-12)
    np.testing.assert_allclose(sy, y, atol=1e-12)
    # half a pixel above row 0 is the pole; a pixel further the direction comes down the far side
    np.testing.assert_allclose(sr.dir_(3.0, -0.5, H, W), [0, 1, 0], atol=1e-15)
    np.testing.assert_allclose(sr.dir_(3.0, -1.0, H, W), sr.dir_(3.0 + W / 2, 0.0, H, W), atol=1e-15)


def test_rotating_by_the_identity_reproduces_the_frame():
    """R = I on an f32 frame: within 8 d32, d32 = max|restate(f32) - restate(f64)| of this very call."""
    frame = sr.texture(5, 33, 66, 3)[None]
    out64 = sr.equirect_rotate(frame, np.eye(3)[None])
    d32 = float(np.max(np.abs(sr.equirect_rotate(frame, np.eye(3)[None], np.float32) - out64)))
    err = float(np.max(np.abs(out64 - frame)))
    print('identity rotate: max|out - frame| = %.2e, d32 = %.2e' % (err, d32))
    assert 0 < d32 < 1e-4 and err <= 8 * d32


@pytest.mark.parametrize('hw', [(32, 64), (33, 66)])
def test_seam_and_poles_of_a_rotated_analytic_pattern(hw):
    """f = 0.5 + 0.5 sin(k theta) cos(l phi) sampled at the pixel centres and rotated: the seam columns and both pole rows match
    f at the rotated directions within the error of bilinear interpolation, h_theta^2 / 8 max|f_theta_theta| + h_phi^2 / 8
    max|f_phi_phi| with the pitches h_theta = 2 pi / W, h_phi = pi / H; where the sample lies between a pole and the first row
    of pixel centres the row is replicated, which adds |phi' - phi_row| <= h_phi / 2 times max|f_phi| over that cap."""
    H, W = hw
    k, l = 3, 2
    f = lambda th, ph: 0.5 + 0.5 * np.sin(k * th) * np.cos(l * ph)
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    th = (2 * (x + 0.5) / W - 1) * np.pi
    ph = (1 - 2 * (y + 0.5) / H) * np.pi / 2
    R = sr.rot(sr.AXIS, np.deg2rad(7.0))
    got = sr.equirect_rotate(f(th, ph)[None, ..., None], R[None])[0, ..., 0]
    q = sr.dir_(x, y, H, W) @ R.T
    th2, ph2 = np.arctan2(q[..., 2], q[..., 0]), np.arcsin(np.clip(q[..., 1], -1, 1))
    h_th, h_ph = 2 * np.pi / W, np.pi / H
    e2 = h_th ** 2 / 8 * 0.5 * k * k + h_ph ** 2 / 8 * 0.5 * l * l
    cap = np.abs(ph2) > np.pi / 2 - h_ph / 2
    f_phi_cap = 0.5 * l * float(np.max(np.abs(np.sin(l * (np.pi / 2 - np.linspace(0, h_ph / 2, 65))))))
    tol = e2 + cap * (h_ph / 2) * f_phi_cap
    err = np.abs(got - f(th2, ph2))
    sx, _ = sr.pix(q, H, W)
    assert cap[[0, -1]].any() and (np.floor(sx) < 0).any() and (np.floor(sx) >= W - 1).any()      # the paths are taken
    for name, sel in (('seam', (slice(None), [0, W - 1])), ('poles', ([0, H - 1], slice(None)))):
        print('%s %s: max err %.2e (bound %.2e .. %.2e)' % (name, hw, err[sel].max(), tol[sel].min(), tol[sel].max()))
        assert np.all(err[sel] <= tol[sel])
    assert np.all(err <= tol)
    # the seam is continuous: columns W - 1 and 0 of the result differ like any two neighbours
    assert np.max(np.abs(got[:, 0] - got[:, -1])) <= 1.5 * np.max(np.abs(np.diff(got, axis=1)))


def test_composition():
    R = np.stack([sr.rot(sr.AXIS, 0.02), sr.rot((0, 1, 0), -0.05), sr.rot((1, 0, 0), 0.01)])
    Cs = sr.compose(R)
    assert Cs.shape == (4, 3, 3) and np.array_equal(Cs[0], np.eye(3))
    np.testing.assert_allclose(Cs[3], R[2] @ R[1] @ R[0], atol=1e-15)
    for Cm in Cs:
        np.testing.assert_allclose(Cm @ Cm.T, np.eye(3), atol=1e-15)
    assert np.array_equal(sr.compose(np.stack([np.eye(3)] * 3)), np.stack([np.eye(3)] * 4))       # exact on I
    from cp_360_weakly_supervised_saliency_amd.utils import stabilize
    np.testing.assert_array_equal(stabilize.compose(R.astype(np.float32)), sr.compose(R.astype(np.float32)))


def test_singular_and_non_finite_inputs():
    """A single pixel (N of rank 2) and all-NaN flow leave R = I with the sum of weights 0; NaN pixels weigh 0."""
    R, d = sr.rotation_fit(np.zeros((1, 1, 2)))
    assert np.array_equal(R, np.eye(3)) and d[1] == 0
    R, d = sr.rotation_fit(np.full((8, 16, 2), np.nan))
    assert np.array_equal(R, np.eye(3)) and d[1] == 0
    R_true = sr.rot(sr.AXIS, 0.03)
    flow = sr.rotation_flow(R_true, 16, 32)
    holes = np.zeros((16, 32), bool)
    holes[3:9, 5:20] = True
    bad = flow.copy()
    bad[holes] = np.nan
    assert np.array_equal(sr.rotation_fit(bad)[0], sr.rotation_fit(flow, weight0=holes)[0])
    assert np.max(np.abs(sr.rotation_fit(bad)[0] - R_true)) <= 1e-9


def test_status_codes_without_gpu():
    """Argument validation happens before any launch (following tests/test_abi.py)."""
    L = _lib.lib()
    one = C.c_void_p(16)
    a16 = lambda n: (n + 15) & ~15
    # tables f32 [W][2] + [H][2]; per pair 16 doubles of state and one partial of 12 doubles per 2048 pixels
    assert L.cp360_stab_work_bytes(0, 480, 960) == 8 * 960 + 8 * 480
    assert L.cp360_stab_work_bytes(0, 33, 67) == a16(8 * 67) + a16(8 * 33)
    assert L.cp360_stab_work_bytes(3, 480, 960) == 8 * 1440 + 3 * 8 * (16 + 12 * 225)
    assert L.cp360_stab_work_bytes(2, 33, 66) == a16(8 * 66) + a16(8 * 33) + 2 * 8 * (16 + 12 * 2)
    assert L.cp360_stab_work_bytes(-1, 4, 8) == 0 and L.cp360_stab_work_bytes(1, 0, 8) == 0 and L.cp360_stab_work_bytes(1, 4, -8) == 0
    big = 1 << 20
    fit = lambda flow, F, H, W, iters, cmin, R, diag, work, nbytes: L.cp360_stab_fit(flow, F, H, W, iters, cmin, R, diag, work, nbytes, None)
    # every call below fails its checks before anything is launched: the dummy pointers are never used
    assert fit(None, 1, 16, 32, 8, 0.25, one, one, one, big) == -5
    assert fit(one, 1, 16, 32, 8, 0.25, None, one, one, big) == -5
    assert fit(one, 1, 16, 32, 8, 0.25, one, None, one, big) == -5
    assert fit(one, 1, 16, 32, 8, 0.25, one, one, None, big) == -5
    assert fit(one, 0, 16, 32, 8, 0.25, one, one, one, big) == -1
    assert fit(one, 1, 0, 32, 8, 0.25, one, one, one, big) == -1
    assert fit(one, 1, 16, -1, 8, 0.25, one, one, one, big) == -1
    assert fit(one, 1, 16, 32, 0, 0.25, one, one, one, big) == -1                    # iters < 1
    assert fit(one, 1, 16, 32, 8, 0.0, one, one, one, big) == -1                     # c_min_px
    assert fit(one, 1, 16, 32, 8, 0.25, one, one, one, L.cp360_stab_work_bytes(1, 16, 32) - 1) == -1      # workspace too small
    assert fit(one, 1, 16, 32, 8, 0.25, one, one, C.c_void_p(8), big) == -6          # workspace alignment
    assert fit(one, 70000, 16, 32, 8, 0.25, one, one, one, 1 << 40) == -8
    assert L.cp360_stab_flow(None, 1, 16, 32, one, one, big, None) == -5
    assert L.cp360_stab_flow(one, 1, 16, 32, None, one, big, None) == -5
    assert L.cp360_stab_flow(one, 1, 16, 32, one, None, big, None) == -5
    assert L.cp360_stab_flow(one, 0, 16, 32, one, one, big, None) == -1
    assert L.cp360_stab_flow(one, 1, 16, 0, one, one, big, None) == -1
    assert L.cp360_stab_flow(one, 1, 16, 32, one, one, 8 * 48 - 1, None) == -1
    rot = lambda dt, fr, R, N, H, W, Cn, out, work, nbytes: L.cp360_stab_rotate(dt, fr, R, N, H, W, Cn, out, work, nbytes, None)
    two = C.c_void_p(32)
    assert rot(_lib.F32, None, one, 1, 16, 32, 3, two, one, big) == -5
    assert rot(_lib.F32, one, None, 1, 16, 32, 3, two, one, big) == -5
    assert rot(_lib.F32, one, one, 1, 16, 32, 3, None, one, big) == -5
    assert rot(_lib.F32, one, one, 1, 16, 32, 3, two, None, big) == -5
    assert rot(_lib.F32, one, one, 0, 16, 32, 3, two, one, big) == -1
    assert rot(_lib.F32, one, one, 1, 16, 32, 0, two, one, big) == -1
    assert rot(_lib.F32, one, one, 1, 16, 32, 5, two, one, big) == -8                # C > 4
    assert rot(_lib.U8, one, one, 1, 16, 32, 4, two, one, big) == -8                 # u8 frames are RGB
    assert rot(_lib.BF16, one, one, 1, 16, 32, 3, two, one, big) == -4
    assert rot(_lib.F32, one, one, 1, 16, 32, 3, one, one, big) == -8                # in place
    assert rot(_lib.F32, one, one, 1, 16, 32, 3, two, one, 8 * 48 - 1) == -1         # workspace too small


@pytest.mark.parametrize('name, size', [('_stab_work', 'cp360_stab_work_bytes'), ('_shot_work', 'cp360_shot_work_bytes'),
                                        ('sphere_eval_work', 'cp360_seval_work_bytes'), ('fixation_work', 'cp360_fix_work_bytes')])
def test_a_workspace_is_kept_only_when_it_owns_the_bytes_the_library_is_told(name, size):
    """The ops hand the library work.numel() * 8 as the workspace's byte count.  So, of a caller's tensors, only a float64 one of
    at least the needed bytes is used as it is; one 8 bytes short, and a float32 or a uint8 one of the same numel() (which own a
    half and an eighth of the bytes that count claims), are replaced by a float64 tensor that is large enough.  The sizes come
    from the host functions cp360_*_work_bytes: no GPU."""
    import torch
    from cp_360_weakly_supervised_saliency_amd import ops
    get, cpu = getattr(ops, name), torch.device('cpu')
    F, h, w = 1, 16, 32
    need = getattr(_lib.lib(), size)(F, h, w)
    assert need > 0 and need % 8 == 0
    fresh = get(F, h, w, cpu)
    assert fresh.dtype == torch.float64 and fresh.device == cpu and fresh.numel() * 8 == need
    exact = torch.empty(need // 8, dtype=torch.float64)
    assert get(F, h, w, cpu, exact) is exact
    for bad in (torch.empty(need // 8 - 1, dtype=torch.float64), torch.empty(need // 8, dtype=torch.float32),
                torch.empty(need // 8, dtype=torch.uint8)):
        got = get(F, h, w, cpu, bad)
        assert got is not bad and got.dtype == torch.float64 and got.device == cpu and got.is_contiguous()
        assert got.numel() * got.element_size() >= need
    with pytest.raises(ValueError, match='unsupported geometry'):
        get(70000, h, w, cpu)


def test_ops_refuse_bad_arguments_without_gpu():
    import torch
    from cp_360_weakly_supervised_saliency_amd import ops
    with pytest.raises(RuntimeError):
        ops.rotation_fit(torch.zeros(1, 8, 16, 2))
    with pytest.raises(RuntimeError):
        ops.rotation_flow(torch.eye(3)[None], 8, 16)
    with pytest.raises(RuntimeError):
        ops.equirect_rotate(torch.zeros(1, 8, 16, 3), torch.eye(3)[None])
