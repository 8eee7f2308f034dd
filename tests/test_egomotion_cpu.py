"""The specification of the ego-motion fit and the independent-motion flow (K23) on the CPU: the claims of its
float64 restatement (tests/egomotion_restate.py) that the GPU tests then rest on, and the argument checks of the C entry points
and of the wrappers, which need no GPU.

Bounds.  The fixed conditions are the issue's: the direction of e within 1 degree, the rotation better than K11's fit alone on the
same flow.  The tight ones are twice what the restatement measured on these very scenes (MEASURED below, recorded in DESIGN 7o);
the flows are deterministic (hash RNG), so a change of the definition shows up here first.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from cp_360_weakly_supervised_saliency_amd import _lib
from tests import egomotion_restate as er
from tests import stabilize_restate as sr

MOVE = 2.5                       # the mover's own motion in grid pixels
SMALL = dict(c_min_px=0.05, t_min_px=0.05)          # at 32 x 64 a pixel is 5.6 degrees: thresholds of 0.28 degree
# (hw, t, noise, mover) -> (error of e in degrees, error of R in degrees) of the float64 restatement
MEASURED = {
    ((32, 64), 0.3, 0, 0): (0.00022, 8.13e-05), ((32, 64), 0.3, 0, 1): (0.000752, 0.000292),
    ((32, 64), 0.3, 1, 0): (0.133, 0.0804), ((32, 64), 0.3, 1, 1): (0.161, 0.0805),
    ((120, 240), 0.02, 0, 0): (0.000849, 2.46e-06), ((120, 240), 0.02, 0, 1): (0.0434, 0.000146),
    ((120, 240), 0.02, 1, 0): (0.2, 0.00119), ((120, 240), 0.02, 1, 1): (0.249, 0.00126),
    ((120, 240), 0.1, 0, 0): (0.000412, 9.6e-06), ((120, 240), 0.1, 0, 1): (0.00215, 0.000195),
    ((120, 240), 0.1, 1, 0): (0.00989, 0.00134), ((120, 240), 0.1, 1, 1): (0.0147, 0.00146),
    ((120, 240), 0.3, 0, 0): (0.000316, 4.26e-05), ((120, 240), 0.3, 0, 1): (0.000806, 0.000344),
    ((120, 240), 0.3, 1, 0): (0.00304, 0.0013), ((120, 240), 0.3, 1, 1): (0.00597, 0.00149),
}
CASES = [((32, 64), 0.3)] + [((120, 240), t) for t in (0.02, 0.1, 0.3)]


def fit_kwargs(hw, t):
    if hw[0] < 100:
        return SMALL
    return dict(t_min_px=0.05) if t < 0.05 else {}          # 0.02 of translation moves little by 0.25 px at 120 x 240


@functools.lru_cache(maxsize=None)
def fit_case(hw, t, noise, mover):
    flow, static, R_true = er.scene_flow(hw[0], hw[1], t, noise_px=0.05 if noise else 0.0, seed=7, mover=(MOVE, 0.0) if mover else None)
    flow = flow.astype(np.float32)
    kw = fit_kwargs(hw, t)
    R0 = sr.rotation_fit(flow, 8, kw.get('c_min_px', 0.25))[0]
    R, e, D = er.egomotion_fit(flow, **kw)
    return flow, static, R_true, R0, R, e, D


@pytest.mark.parametrize('mover', [0, 1])
@pytest.mark.parametrize('noise', [0, 1])
@pytest.mark.parametrize('hw,t', CASES)
def test_fit_recovers_direction_and_rotation(hw, t, noise, mover):
    flow, static, R_true, R0, R, e, D = fit_case(hw, t, noise, mover)
    err_e = er.angle_deg(e, er.E_TRUE)
    err_R, err_R0 = np.degrees(sr.angle_between(R, R_true)), np.degrees(sr.angle_between(R0, R_true))
    print('MEASURED (%s, %s, %d, %d): (%.3g, %.3g),   K11 alone %.4f deg, diag %s' % (hw, t, noise, mover, err_e, err_R, err_R0, D))
    assert D[7] == er.OK and abs(np.linalg.norm(e) - 1.0) <= 1e-12
    np.testing.assert_allclose(R @ R.T, np.eye(3), atol=4e-7)          # R = R0 (held in float32) times exact rotations
    assert err_e < 1.0
    assert err_R < err_R0
    m_e, m_R = MEASURED[(hw, t, noise, mover)]
    assert err_e <= 2 * m_e and err_R <= 2 * m_R


def test_background_mover_and_false_alarms():
    """t = 0.1 at 120 x 240, 0.05 px of noise and the mover.  Measured: p95 of mag over the static pixels 0.0885 px against 2.30 px
    of the de-rotated flow (ratio 0.038) and 0.0884 px under the true (R, e); the mover's median 2.499 px of its 2.5 px; no static
    pixel above 0.25 px, under the fit and under the truth."""
    flow, static, R_true, R0, R, e, D = fit_case((120, 240), 0.1, 1, 1)
    res, mag = er.egomotion_residual(flow, R, e)
    derot = er.egomotion_residual(flow, R, np.zeros(3))[1]
    truth = er.egomotion_residual(flow, R_true, er.E_TRUE)[1]
    p95, p95_derot, p95_true = (float(np.percentile(m[static], 95)) for m in (mag, derot, truth))
    med = float(np.median(mag[~static]))
    fa, fa_true = float(np.mean(mag[static] > 0.25)), float(np.mean(truth[static] > 0.25))
    print('static p95 %.4f px (de-rotated %.4f, ratio %.4f; true camera %.4f), mover median %.4f of %.1f px, false alarms %.4f '
          '(true camera %.4f)' % (p95, p95_derot, p95 / p95_derot, p95_true, med, MOVE, fa, fa_true))
    assert p95 < 0.1 * p95_derot
    assert p95 <= 2 * p95_true
    assert med >= 0.8 * MOVE
    assert fa_true < 0.05 and fa < 0.05
    np.testing.assert_allclose(np.hypot(res[..., 0] * np.cos(np.pi * (0.5 - (np.arange(120) + 0.5) / 120))[:, None], res[..., 1])[40:80],
                               mag[40:80], rtol=0.05, atol=0.02)      # res is mag's flow (compared away from the poles)


def test_gate_keeps_a_stationary_camera_still():
    """A camera that only turns, with the mover: the gate closes (e = 0 exactly, R = R0 bit for bit, res the de-rotated flow, share
    the mover's weighted area).  With min_share = 0 the fit runs and explains the mover away: the failure the gate exists for
    (measured: the mover's median mag falls from 2.5 px to 0.69 px; asserted: below half of its motion)."""
    H, W = 120, 240
    flow, static, R_true = er.scene_flow(H, W, 0.0, mover=(MOVE, 0.0))
    flow = flow.astype(np.float32)
    R0 = sr.rotation_fit(flow)[0].astype(np.float32).astype(np.float64)
    R, e, D = er.egomotion_fit(flow)
    assert D[7] == er.GATED and np.array_equal(e, np.zeros(3)) and np.array_equal(R, R0)
    a = np.broadcast_to(sr.tables(H, W)[2][:, None], (H, W))
    assert abs(D[0] - a[~static].sum() / a.sum()) <= 1e-12
    res, mag = er.egomotion_residual(flow, R, e)
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    g = sr.dir_(xs + flow[..., 0].astype(np.float64), ys + flow[..., 1].astype(np.float64), H, W) @ R0
    sx, sy = sr.pix(g, H, W)
    np.testing.assert_allclose(res, np.stack([er._wrap(sx - xs, W, np.float64), sy - ys], -1), atol=1e-9)
    assert np.median(mag[~static]) >= 0.95 * MOVE
    R2, e2, D2 = er.egomotion_fit(flow, min_share=0.0)
    mag2 = er.egomotion_residual(flow, R2, e2)[1]
    print('stationary camera: share %.5f; without the gate the mover keeps a median of %.4f px of %.1f' % (D[0], np.median(mag2[~static]), MOVE))
    assert D2[7] == er.OK and np.median(mag2[~static]) < 0.5 * MOVE


def test_chirality():
    """A patch of sky that moves along its epipolar lines: toward +e no static point can, so the motion stays as residual; away
    from +e it is a nearer static point, and is absorbed."""
    H, W = 120, 240
    for along, keeps in ((-MOVE, True), (MOVE, False)):
        flow, static, R_true = er.scene_flow(H, W, 0.1, noise_px=0.05, seed=7, mover=(0.0, along))
        flow = flow.astype(np.float32)
        R, e, D = er.egomotion_fit(flow)
        mag = er.egomotion_residual(flow, R, e)[1]
        med = float(np.median(mag[~static]))
        print('patch moving %+.1f px along its epipolar lines: median mag %.4f px, e within %.4f deg' % (along, med, er.angle_deg(e, er.E_TRUE)))
        assert er.angle_deg(e, er.E_TRUE) < 1.0
        assert med >= 0.8 * MOVE if keeps else med <= 0.1 * MOVE


def test_symmetries():
    H, W = 120, 240
    flow, static, R_true, R0, R, e, D = fit_case((120, 240), 0.1, 1, 1)
    # T -> -T flips e
    back = er.scene_flow(H, W, 0.1, e_true=-er.E_TRUE, noise_px=0.05, seed=7, mover=(MOVE, 0.0))[0].astype(np.float32)
    e_back = er.egomotion_fit(back)[1]
    assert er.angle_deg(e_back, -er.E_TRUE) < 2 * MEASURED[((120, 240), 0.1, 1, 1)][0]
    # a yaw by whole columns rolls the flow: e and R turn with it, res rolls.  A quarter turn (W / 4 columns) permutes the axes with
    # signs, so the float32 rounding of R0, R and e that the definition contains turns with it too, and 1e-9 holds end to end
    k = W // 4
    Y = np.rint(sr.rot((0, 1, 0), -2 * np.pi * k / W))      # theta -> theta + 2 pi k / W
    np.testing.assert_allclose(sr.dir_(5 + k, 9, H, W), Y @ sr.dir_(5, 9, H, W), atol=1e-15)
    flow_y = np.roll(flow, k, axis=1)
    Ry, ey, Dy = er.egomotion_fit(flow_y)
    np.testing.assert_allclose(ey, Y @ e, atol=1e-9)
    np.testing.assert_allclose(Ry, Y @ R @ Y.T, atol=1e-9)
    np.testing.assert_allclose(Dy, D, rtol=1e-9, atol=1e-12)
    R32, e32 = R.astype(np.float32).astype(np.float64), e.astype(np.float32).astype(np.float64)
    np.testing.assert_allclose(np.roll(er.egomotion_residual(flow, R32, e32)[0], k, axis=1),
                               er.egomotion_residual(flow_y, Y @ R32 @ Y.T, Y @ e32)[0], atol=1e-9)
    # a pure rotation closes the gate
    turn = er.scene_flow(H, W, 0.0)[0].astype(np.float32)
    Rt, et, Dt = er.egomotion_fit(turn)
    assert Dt[7] == er.GATED and Dt[0] == 0.0 and np.array_equal(et, np.zeros(3))
    assert np.degrees(sr.angle_between(Rt, R_true)) < 1e-4
    # a pure translation keeps R at the identity
    flow_t = er.scene_flow(H, W, 0.1, R_true=np.eye(3), noise_px=0.05, seed=7)[0].astype(np.float32)
    Ri, ei, Di = er.egomotion_fit(flow_t)
    err = np.degrees(sr.angle_between(Ri, np.eye(3)))
    print('pure translation: R within %.5f deg of I, e within %.4f deg' % (err, er.angle_deg(ei, er.E_TRUE)))
    assert err <= 2 * MEASURED[((120, 240), 0.1, 1, 0)][1] and er.angle_deg(ei, er.E_TRUE) <= 2 * MEASURED[((120, 240), 0.1, 1, 0)][0]


def test_odd_inputs_of_the_residual():
    H, W = 32, 64
    ppd = W / 360.0
    e = sr.dir_(40, 11, H, W).astype(np.float32).astype(np.float64)     # an epipole on a pixel centre (and -e on another), as float32 holds it
    tol = 1e-5                                              # float32's rounding of e: 6e-8 rad, times 10 px / rad, times the geometry
    flow = 0.7 * np.ones((H, W, 2))
    res, mag = er.egomotion_residual(flow, np.eye(3), e)
    assert np.array_equal(res[11, 40], [0, 0]) and mag[11, 40] == 0 and np.array_equal(res[H - 1 - 11, 40 - W // 2], [0, 0])
    assert np.count_nonzero(mag == 0) == 2
    # clamped at 0: 3 degrees toward +e stay as 3 degrees; clamped at alpha_max: 20 degrees away from +e stop at -e
    fl, to_anti = er.arc_flow(H, W, e, -3.0)
    mag = er.egomotion_residual(fl, np.eye(3), e)[1]
    ok = to_anti < 179
    np.testing.assert_allclose(mag[ok & (to_anti > 4)], 3.0 * ppd, atol=tol)
    fl, to_anti = er.arc_flow(H, W, e, 20.0)
    res, mag = er.egomotion_residual(fl, np.eye(3), e)
    near = (to_anti < 20) & (to_anti > 1e-3)
    assert near.sum() >= 5
    np.testing.assert_allclose(mag[near], (20.0 - to_anti[near]) * ppd, atol=tol)
    np.testing.assert_allclose(mag[to_anti > 20.5], 0.0, atol=tol)
    # NaN and infinity in single pixels: NaN there, and nothing else moves
    bad = fl.copy()
    bad[3, 5, 0], bad[20, 63, 1], bad[31, 0] = np.nan, np.inf, (-np.inf, np.nan)
    res_b, mag_b = er.egomotion_residual(bad, np.eye(3), e)
    hole = np.zeros((H, W), bool)
    hole[3, 5] = hole[20, 63] = hole[31, 0] = True
    assert np.all(np.isnan(res_b[hole])) and np.all(np.isnan(mag_b[hole]))
    assert np.array_equal(res_b[~hole], res[~hole]) and np.array_equal(mag_b[~hole], mag[~hole])


def test_odd_inputs_of_the_fit():
    flow, static, R_true, R0, R, e, D = fit_case((32, 64), 0.3, 1, 1)
    bad, bad2 = flow.copy(), flow.copy()
    for b, v in ((bad, np.nan), (bad2, np.inf)):
        b[3, 5, 0], b[20, 63, 1], b[31, 0] = v, v, (v, -v)
    Rb, eb, Db = er.egomotion_fit(bad, **SMALL)
    Rc, ec, Dc = er.egomotion_fit(bad2, **SMALL)
    assert np.array_equal(Rb, Rc) and np.array_equal(eb, ec) and np.array_equal(Db, Dc)      # non-finite is non-finite
    assert np.all(np.isfinite(Rb)) and np.all(np.isfinite(Db)) and er.angle_deg(eb, er.E_TRUE) < 1.0
    assert Db[1] < D[1]                                                                    # their weight is gone
    R0g = sr.rot(sr.AXIS, 0.01)
    R0f = R0g.astype(np.float32).astype(np.float64)
    for what, fl in (('all NaN', np.full((8, 16, 2), np.nan)), ('1 x 1', np.ones((1, 1, 2))), ('zero', np.zeros((8, 16, 2))),
                     ('zero, no gate', np.zeros((8, 16, 2)))):
        kw = dict(min_share=0.0) if 'no gate' in what else {}
        Rz, ez, Dz = er.egomotion_fit(fl, R0=np.eye(3) if 'zero' in what else R0g, **kw)
        assert np.array_equal(ez, np.zeros(3)) and Dz[7] != er.OK and Dz[1] == 0, what
        assert np.array_equal(Rz, np.eye(3) if 'zero' in what else R0f), what
    assert er.egomotion_fit(np.zeros((8, 16, 2)), R0=np.eye(3), min_share=0.0)[2][7] == er.SINGULAR
    assert er.egomotion_fit(np.zeros((8, 16, 2)))[2][7] == er.GATED


def test_eigen_solve_against_eigh():
    """The scalar Jacobi routine on every M of the scenes above, and on the same matrices with a tenfold smaller gap between the
    two small eigenvalues: eigenvalues within 8 eps lambda_2, the eigenvector within 32 eps lambda_2 / gap of LAPACK's (the first-order
    bound of an eigenvector under a perturbation of norm 32 eps lambda_2)."""
    eps = np.finfo(np.float64).eps
    mats = []
    for hw, t in CASES:
        trace = []
        flow = fit_case(hw, t, 1, 1)[0]
        er.egomotion_fit(flow, trace=trace, **fit_kwargs(hw, t))
        mats += [m for _, _, m in trace]
    assert len(mats) == 8 * len(CASES)
    worst = 0.0
    for m in mats:
        M = np.array([[m[0], m[1], m[2]], [m[1], m[3], m[4]], [m[2], m[4], m[5]]])
        lam, V = np.linalg.eigh(M)
        for shrink in (1.0, 0.1):
            Ms = (V * np.array([lam[0], lam[0] + shrink * (lam[1] - lam[0]), lam[2]])) @ V.T
            Ms = 0.5 * (Ms + Ms.T)
            want, Vs = np.linalg.eigh(Ms)
            got, v = er.eig3_jacobi((Ms[0, 0], Ms[0, 1], Ms[0, 2], Ms[1, 1], Ms[1, 2], Ms[2, 2]))
            assert np.all(np.abs(got - want) <= 8 * eps * want[2])
            ang = np.arcsin(min(1.0, np.linalg.norm(np.cross(v, Vs[:, 0]))))
            worst = max(worst, ang * (want[1] - want[0]) / (eps * want[2]))
            assert ang <= 32 * eps * want[2] / (want[1] - want[0]), (m, shrink)
            assert abs(np.linalg.norm(v) - 1) <= 4 * eps
    print('eigenvector error at most %.2f eps lambda_2 / gap over %d matrices' % (worst, 2 * len(mats)))
    # fewer sweeps are not enough everywhere, the chosen count has a margin: 4 sweeps already reach the bound on these
    for m in mats:
        assert np.allclose(er.eig3_jacobi(m, 4)[0], er.eig3_jacobi(m)[0], rtol=0, atol=8 * eps * er.eig3_jacobi(m)[0][2])


def test_exports_and_status_codes_without_gpu():
    """Argument validation happens before any launch (following tests/test_stabilize_cpu.py): the dummy pointers are never used."""
    L = _lib.lib()
    assert L.cp360_version() == 306 == _lib.ABI_VERSION
    for name in ('cp360_ego_work_bytes', 'cp360_ego_fit', 'cp360_ego_residual'):
        assert hasattr(L, name) and name in _lib.PUBLIC_SYMBOLS
    one, two = C.c_void_p(16), C.c_void_p(32)
    a16 = lambda n: (n + 15) & ~15
    # tables f32 [W][2] + [H][2]; per pair 32 doubles of state and one partial of 24 doubles per 2048 pixels
    assert L.cp360_ego_work_bytes(0, 480, 960) == 8 * 1440 == L.cp360_stab_work_bytes(0, 480, 960)
    assert L.cp360_ego_work_bytes(3, 480, 960) == 8 * 1440 + 3 * 8 * (32 + 24 * 225)
    assert L.cp360_ego_work_bytes(2, 33, 66) == a16(8 * 66) + a16(8 * 33) + 2 * 8 * (32 + 24 * 2)
    for F, H, W in ((1, 1, 1), (3, 16, 32), (2, 33, 66), (64, 480, 960)):
        assert L.cp360_ego_work_bytes(F, H, W) >= L.cp360_stab_work_bytes(F, H, W) > 0        # K11's start runs in it
    assert L.cp360_ego_work_bytes(-1, 4, 8) == 0 and L.cp360_ego_work_bytes(1, 0, 8) == 0 and L.cp360_ego_work_bytes(1, 4, -8) == 0
    assert L.cp360_ego_work_bytes(70000, 4, 8) == 0
    big = 1 << 20

    def fit(flow=one, R0=one, F=1, H=16, W=32, iters=8, cmin=0.25, tmin=0.25, share=0.25, R=one, e=one, diag=one, work=one, nbytes=big):
        return L.cp360_ego_fit(flow, R0, F, H, W, iters, cmin, tmin, share, R, e, diag, work, nbytes, None)
    for k in ('flow', 'R0', 'R', 'e', 'diag', 'work'):
        assert fit(**{k: None}) == -5, k
    assert fit(F=0) == -1 and fit(H=0) == -1 and fit(W=-1) == -1 and fit(iters=0) == -1
    assert fit(cmin=0.0) == -1 and fit(cmin=float('nan')) == -1 and fit(tmin=-1.0) == -1 and fit(tmin=float('inf')) == -1
    assert fit(share=-0.1) == -1 and fit(share=float('nan')) == -1
    assert fit(nbytes=L.cp360_ego_work_bytes(1, 16, 32) - 1) == -1                  # workspace too small
    assert fit(work=C.c_void_p(8)) == -6                                            # workspace alignment
    assert fit(F=70000, nbytes=1 << 40) == -8

    def residual(flow=one, R=one, e=one, F=1, H=16, W=32, res=two, mag=two, work=one, nbytes=big):
        return L.cp360_ego_residual(flow, R, e, F, H, W, res, mag, work, nbytes, None)
    for k in ('flow', 'R', 'e', 'res', 'work'):
        assert residual(**{k: None}) == -5, k
    assert residual(F=0) == -1 and residual(H=0) == -1 and residual(W=0) == -1
    assert residual(nbytes=8 * 48 - 1) == -1 and residual(work=C.c_void_p(8)) == -6 and residual(F=70000) == -8


def test_ops_refuse_bad_arguments_without_gpu():
    import torch
    from cp_360_weakly_supervised_saliency_amd import ops
    flow, eye, e = torch.zeros(1, 8, 16, 2), torch.eye(3)[None], torch.zeros(1, 3)
    with pytest.raises(RuntimeError):
        ops.egomotion_fit(flow)                              # a CPU tensor: there is no CPU fallback
    with pytest.raises(RuntimeError):
        ops.egomotion_fit(flow, R0=eye)
    with pytest.raises(RuntimeError):
        ops.egomotion_residual(flow, eye, e)
    # the checks of shape, type and layout come before anything is launched; a meta tensor passes for a device tensor
    meta = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device='meta')
    from unittest import mock
    with mock.patch.object(ops, 'require_gpu', lambda *a: None):
        for bad in (meta(8, 16, 2), meta(1, 8, 16, 3), meta(1, 8, 16, 2, dtype=torch.float64), meta(1, 8, 32, 2)[:, :, ::2], meta(0, 8, 16, 2)):
            with pytest.raises(ValueError):
                ops.egomotion_fit(bad, R0=meta(1, 3, 3))
            with pytest.raises(ValueError):
                ops.egomotion_residual(bad, meta(1, 3, 3), meta(1, 3))
        with pytest.raises(ValueError):
            ops.egomotion_fit(meta(1, 8, 16, 2), R0=meta(1, 3, 3), iters=0)
        with pytest.raises(ValueError):
            ops.egomotion_fit(meta(1, 8, 16, 2), R0=meta(1, 3, 3), min_share=-1.0)
        with pytest.raises(ValueError):
            ops.egomotion_fit(meta(1, 8, 16, 2), R0=meta(2, 3, 3))
        with pytest.raises(ValueError):
            ops.egomotion_fit(meta(1, 8, 16, 2), R0=meta(1, 3, 3, dtype=torch.float64))
        with pytest.raises(ValueError, match="device"):
            ops.egomotion_fit(meta(1, 8, 16, 2), R0=eye)                             # R0 on another device than the flow
        with pytest.raises(ValueError, match="device"):
            ops.egomotion_residual(meta(1, 8, 16, 2), eye, meta(1, 3))
        with pytest.raises(ValueError):
            ops.egomotion_residual(meta(1, 8, 16, 2), meta(1, 3, 3), meta(1, 4))
        with pytest.raises(ValueError):
            ops.egomotion_residual(meta(1, 8, 16, 2), meta(1, 3, 3), meta(1, 3), out=meta(1, 8, 16, 3))
