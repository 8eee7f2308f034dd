"""360-degree stabilisation on the GPU (K11, csrc/stabilize.hip) against the float64 restatement of its specification
(tests/stabilize_restate.py, whose own claims tests/test_stabilize_cpu.py pins) on the same float32 inputs.

Bounds.  The kernels evaluate every per-pixel term in float32 and every sum in float64; the restatement does the same with
``dtype=np.float32``, operation by operation, so d32 = max|restate(f32) - restate(f64)| on an input is the size of float32's
roundings on it and the device is held to 8 d32, plus 2^-22 of the result's scale where the result itself is stored as float32
(a rotation matrix has entries up to 1; the diagnostics are compared relative to max(1, |value|)).  Horizontal displacements
live on a circle of W pixels: they are compared modulo W, since a pixel carried half-way round sits on the wrap of
[-W / 2, W / 2), where the last bit decides the sign.
"""
import functools
import os

import numpy as np
import pytest
import torch

from cp_360_weakly_supervised_saliency_amd import ops
from cp_360_weakly_supervised_saliency_amd.data.dataset import Sal360Dataset
from cp_360_weakly_supervised_saliency_amd.utils import npy_io
from cp_360_weakly_supervised_saliency_amd.utils.stabilize import Stabilizer
from tests import farneback_restate as fb
from tests import stabilize_restate as sr

pytestmark = pytest.mark.gpu
DEV = 'cuda'
FLOOR = 2.0 ** -22


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ----------------------------------------------------------------------------- fit
@functools.lru_cache(maxsize=None)
def fit_case(hw, F=3):
    """F noisy-plus-outlier flows (0.5, 3 and 10 degrees about a non-axis direction; one pair: 3 degrees), the float64 fit and
    d32 of R and of the diagnostics."""
    degs = (3.0,) if F == 1 else (0.5, 3.0, 10.0)[:F]
    flow = np.stack([sr.noisy_outlier_flow(sr.rot(sr.AXIS, np.deg2rad(d)), hw[0], hw[1], 200 + i) for i, d in enumerate(degs)])
    R64, D64 = sr.rotation_fit(flow)
    R32, D32 = sr.rotation_fit(flow, dtype=np.float32)
    return flow, R64, D64, float(np.max(np.abs(R32 - R64))), np.max(np.abs(D32 - D64), 0)


def check_fit(got_R, got_D, R64, D64, dR, dD, what):
    eR = float(np.max(np.abs(got_R - R64)))
    eD = np.max(np.abs(got_D - D64), 0)
    tolD = 8 * dD + FLOOR * np.maximum(1.0, np.max(np.abs(D64), 0))
    print('%s: max|R - R64| = %.2e (d32 %.2e, bound %.2e); diag err %s (bound %s)' % (what, eR, dR, 8 * dR + FLOOR, eD, tolD))
    assert eR <= 8 * dR + FLOOR
    assert np.all(eD <= tolD)


@pytest.mark.parametrize('hw', [(16, 32), (33, 66), (120, 240)])
def test_fit_matches_the_restatement(hw):
    """16 x 32 is one workgroup per pair, 33 x 66 two with a tail, 120 x 240 fifteen partials per pair."""
    flow, R64, D64, dR, dD = fit_case(hw)
    R, D = ops.rotation_fit(dev(flow))
    assert R.shape == (3, 3, 3) and R.dtype == torch.float32 and D.shape == (3, 4) and D.dtype == torch.float64
    check_fit(R.cpu().numpy().astype(np.float64), D.cpu().numpy(), R64, D64, dR, dD, 'fit %s' % (hw,))
    # other parameters travel: 2 iterations and another floor
    R2, D2 = ops.rotation_fit(dev(flow), iters=2, c_min_px=0.5)
    w64, wD = sr.rotation_fit(flow, iters=2, c_min_px=0.5)
    w32, wD32 = sr.rotation_fit(flow, iters=2, c_min_px=0.5, dtype=np.float32)
    check_fit(R2.cpu().numpy().astype(np.float64), D2.cpu().numpy(), w64, wD, float(np.max(np.abs(w32 - w64))),
              np.max(np.abs(wD32 - wD), 0), 'fit %s, 2 iterations' % (hw,))


def test_fit_full_size():
    """One pair at the driver's 480 x 960: 225 partials."""
    flow, R64, D64, dR, dD = fit_case((480, 960), 1)
    R, D = ops.rotation_fit(dev(flow))
    check_fit(R.cpu().numpy().astype(np.float64), D.cpu().numpy(), R64, D64, dR, dD, 'fit 480 x 960')


def test_fit_is_reproducible_and_independent_of_the_batch():
    flow = dev(fit_case((33, 66))[0])
    R, D = ops.rotation_fit(flow)
    R2, D2 = ops.rotation_fit(flow)
    assert torch.equal(R, R2) and torch.equal(D, D2)
    for p in range(3):
        R1, D1 = ops.rotation_fit(flow[p:p + 1])
        assert torch.equal(R1[0], R[p]) and torch.equal(D1[0], D[p])


def test_fit_edge_cases():
    eye = np.eye(3, dtype=np.float32)
    R, D = ops.rotation_fit(torch.zeros(2, 33, 66, 2, device=DEV))
    assert np.array_equal(R.cpu().numpy(), np.stack([eye, eye]))                    # exactly I
    assert np.all(D.cpu().numpy()[:, 2:] == 0) and np.all(D.cpu().numpy()[:, 1] > 0)
    # NaN / inf pixels weigh 0: the restatement with those pixels given zero weight
    flow = fit_case((33, 66))[0][1:2].copy()
    holes = np.zeros((1, 33, 66), bool)
    holes[0, 4:11, 7:30] = True
    holes[0, 32, 65] = True
    bad = flow.copy()
    bad[holes] = np.nan
    bad[0, 5, 9, 0] = np.inf
    bad[0, 6, 9] = (1.0, np.nan)
    R64, D64 = sr.rotation_fit(flow, weight0=holes)
    R32, D32 = sr.rotation_fit(flow, weight0=holes, dtype=np.float32)
    R, D = ops.rotation_fit(dev(bad))
    check_fit(R.cpu().numpy().astype(np.float64), D.cpu().numpy(), R64, D64, float(np.max(np.abs(R32 - R64))),
              np.max(np.abs(D32 - D64), 0), 'fit with NaN pixels')
    # nothing to fit: all NaN, and a single pixel (N of rank 2) -> I, sum of weights 0
    for t in (torch.full((1, 16, 32, 2), float('nan'), device=DEV), torch.zeros(1, 1, 1, 2, device=DEV)):
        R, D = ops.rotation_fit(t)
        assert np.array_equal(R.cpu().numpy()[0], eye) and float(D[0, 1]) == 0.0
    with pytest.raises(ValueError):
        ops.rotation_fit(torch.zeros(1, 16, 32, 2, device=DEV), iters=0)
    with pytest.raises(ValueError):
        ops.rotation_fit(torch.zeros(16, 32, 2, device=DEV))


# ----------------------------------------------------------------------------- rotational flow
def circular(d, W):
    """d with its x component reduced modulo W into [-W / 2, W / 2)."""
    d = d.copy()
    d[..., 0] = np.mod(d[..., 0] + 0.5 * W, W) - 0.5 * W
    return d


@pytest.mark.parametrize('hw', [(16, 32), (33, 66)])
def test_rotation_flow(hw):
    """The identity, a small generic rotation, 40 degrees about the vertical axis (pixels cross the seam) and 25 degrees about
    the x axis (pixels go over a pole, where theta jumps by pi)."""
    check_rotation_flow(hw)


def flow_rotations():
    return np.stack([np.eye(3), sr.rot(sr.AXIS, 0.05), sr.rot((0, 1, 0), np.deg2rad(40.0)), sr.rot((1, 0, 0), np.deg2rad(25.0))])


def leaves_through_the_seam(G):
    """Whether a pixel of the flow G [H, W, 2] lands beyond the first or the last column's centre."""
    x = np.arange(G.shape[1])[None, :]
    return bool(((x + G[..., 0] < -0.5) | (x + G[..., 0] >= G.shape[1] - 0.5)).any())


def goes_over_a_pole(G):
    """Whether a pixel of the flow G [H, W, 2] moves more than a quarter turn in x, as only a path over a pole does."""
    return bool((np.abs(G[..., 0]) > G.shape[1] / 4).any())


def check_rotation_flow(hw, R=None, crossings=True, floor=0.0):
    """R defaults to flow_rotations(); crossings: assert that R[2] leaves through the seam and R[3] goes over a pole; floor: the
    share of the result's scale (max|G|) added to 8 d32, for the rounding of the stored float32."""
    H, W = hw
    R = flow_rotations() if R is None else R
    want = sr.rotation_flow(R, H, W)
    d32 = float(np.max(np.abs(circular(sr.rotation_flow(R, H, W, np.float32) - want, W))))
    if crossings:
        # the cases do what they are for: columns leave through the seam, rows through a pole
        assert leaves_through_the_seam(want[2])
        assert goes_over_a_pole(want[3])
    got = ops.rotation_flow(dev(R.astype(np.float32)), H, W).cpu().numpy()
    assert got.shape == (R.shape[0], H, W, 2) and got.dtype == np.float32
    assert np.all(got[..., 0] >= -W / 2) and np.all(got[..., 0] <= W / 2)
    err = float(np.max(np.abs(circular(got - want, W))))
    tol = 8 * d32 + floor * float(np.max(np.abs(want)))
    print('rotation flow %s: max|d| = %.2e, d32 = %.2e (bound %.2e)' % (hw, err, d32, tol))
    assert err <= tol
    assert float(np.max(np.abs(got[0]))) <= tol
    return got


# ----------------------------------------------------------------------------- resample
def rotations_for(N):
    Rs = [sr.rot(sr.AXIS, 0.06), sr.rot((0, 1, 0), np.deg2rad(40.0)), sr.rot((1, 0.1, 0), np.deg2rad(25.0))]
    return np.stack(Rs[:N])


@pytest.mark.parametrize('hw,N', [((16, 32), 1), ((33, 66), 1), ((64, 128), 3)])
@pytest.mark.parametrize('C', [1, 3, 4])
def test_equirect_rotate_f32(hw, N, C):
    """A box-blurred hash texture; 64 x 128 carries N = 3 frames with a rotation each (generic, across the seam, over a pole)."""
    check_equirect_rotate_f32(hw, rotations_for(N), C)


def f32_frames(hw, N, C):
    return np.stack([3.0 * sr.texture(300 + n, hw[0], hw[1], C) - 1.0 for n in range(N)])


def check_equirect_rotate_f32(hw, R, C):
    frames = f32_frames(hw, R.shape[0], C)
    want = sr.equirect_rotate(frames, R)
    d32 = float(np.max(np.abs(sr.equirect_rotate(frames, R, np.float32) - want)))
    got = ops.equirect_rotate(dev(frames), dev(R.astype(np.float32))).cpu().numpy()
    assert got.shape == frames.shape and got.dtype == np.float32
    err, tol = float(np.max(np.abs(got - want))), 8 * d32 + FLOOR * float(np.max(np.abs(frames)))
    print('rotate f32 %s C %d: max|d| = %.2e (d32 %.2e, bound %.2e)' % (hw, C, err, d32, tol))
    assert err <= tol
    return got


@pytest.mark.parametrize('hw,N', [((33, 66), 1), ((64, 128), 3)])
def test_equirect_rotate_u8(hw, N):
    """At most one level everywhere, and a pixel may differ only where the float64 value before rounding lies within 8 d32 of
    a rounding boundary."""
    frames, R = check_equirect_rotate_u8(hw, rotations_for(N))
    with pytest.raises(ValueError):
        ops.equirect_rotate(dev(frames), dev(R.astype(np.float32)), out=dev(frames)[..., :2])


def u8_frames(hw, N):
    return np.stack([np.rint(255.0 * sr.texture(400 + n, hw[0], hw[1], 3)).astype(np.uint8) for n in range(N)])


def check_u8_against_the_restatement(frames, R, got, what):
    """got u8 = the device's equirect_rotate(frames, R): the two assertions of test_equirect_rotate_u8."""
    raw = sr.equirect_rotate(frames, R, raw=True)
    want = sr.equirect_rotate(frames, R)
    d32 = float(np.max(np.abs(sr.equirect_rotate(frames, R, np.float32, raw=True) - raw)))
    diff = got.astype(np.int32) - want.astype(np.int32)
    to_boundary = np.abs(raw - np.floor(raw) - 0.5)
    print('rotate u8 %s: %d of %d values differ, d32 = %.2e' % (what, np.count_nonzero(diff), diff.size, d32))
    assert np.max(np.abs(diff)) <= 1
    assert np.all(to_boundary[diff != 0] <= 8 * d32)


def check_equirect_rotate_u8(hw, R):
    frames = u8_frames(hw, R.shape[0])
    out = torch.empty(frames.shape, dtype=torch.uint8, device=DEV)
    got = ops.equirect_rotate(dev(frames), dev(R.astype(np.float32)), out=out)
    assert got is out
    check_u8_against_the_restatement(frames, R, got.cpu().numpy(), hw)
    return frames, R


def test_identity_rotations_copy_bit_exactly_through_the_stabilizer():
    """C = I re-renders every u8 frame bit for bit: the sample position of a pixel is its own centre up to float32's rounding
    (below 1e-3 px), which moves a value by less than half a level.  (A video that stands still does not give R = I exactly:
    K10's flow is not zero in the last row and column, where its sample falls out of bounds - DESIGN 7c.)"""
    frames = np.stack([np.rint(255.0 * sr.texture(500 + n, 48, 96, 3)).astype(np.uint8) for n in range(3)])
    eye = np.stack([np.eye(3, dtype=np.float32)] * 3)
    st = Stabilizer((32, 64))
    out = st.render(frames, eye)
    assert out.dtype == torch.uint8 and out.is_cuda and np.array_equal(out.cpu().numpy(), frames)
    np.testing.assert_array_equal(ops.equirect_rotate(dev(frames), dev(eye)).cpu().numpy(), frames)
    # ... and at the driver's width, where a column index has the fewest bits left for the fraction
    wide = np.rint(255.0 * sr.texture(510, 8, 960, 3)).astype(np.uint8)[None]
    np.testing.assert_array_equal(st.render(wide, eye[:1]).cpu().numpy(), wide)
    # frame 0 of stabilize() is a copy whatever the rotations are
    still = np.stack([frames[0]] * 3)
    S, Cm = st.stabilize(still)
    assert np.array_equal(S[0].cpu().numpy(), still[0]) and np.array_equal(Cm[0].cpu().numpy(), eye[0])


# ----------------------------------------------------------------------------- end to end
E2E_HW = (64, 128)


@functools.lru_cache(maxsize=None)
def moving_camera():
    """F = 3: one blurred texture seen by a camera that turns 1 - 2 px-equivalents per step, rendered on the CPU with the
    restatement's resampler in float64 and quantised to u8.  Frame t shows the scene direction p at C_t p, i.e.
    frame_t(q) = scene(C_t^T q).  Returns (frames u8 [4, 64, 128, 3], R_true [3, 3, 3], C_true [4, 3, 3])."""
    H, W = E2E_HW
    px = 2 * np.pi / W
    steps = [sr.rot(sr.AXIS, 1.5 * px), sr.rot((0.1, 1.0, 0.2), -2.0 * px), sr.rot((1.0, 0.2, -0.3), 1.0 * px)]
    C_true = [np.eye(3)]
    for s in steps:
        C_true.append(s @ C_true[-1])
    scene = 255.0 * sr.texture(600, H, W, 3, taps=9).astype(np.float64)
    frames = sr.equirect_rotate(np.stack([scene] * 4), np.stack([c.T for c in C_true]))
    return np.clip(np.rint(frames), 0, 255).astype(np.uint8), np.stack(steps), np.stack(C_true)


@functools.lru_cache(maxsize=None)
def chain_reference():
    """The float64 chain farneback_restate -> stabilize_restate.rotation_fit on the same frames: R [3, 3, 3]."""
    frames = moving_camera()[0]
    return sr.rotation_fit(fb.farneback(fb.gray_from_rgb(frames)))[0]


def weighted_frame_difference(frames):
    """cos phi-weighted mean absolute difference of consecutive frames."""
    f = frames.astype(np.float64)
    w = sr.tables(f.shape[1], f.shape[2])[2][None, :, None, None]
    return float(np.sum(w * np.abs(f[1:] - f[:-1])) / (np.sum(w) * (f.shape[0] - 1) * f.shape[2] * f.shape[3]))


def test_end_to_end_rotations():
    """Stabilizer.rotations recovers every R_t: the device's angular error against the truth is at most twice that of the
    float64 chain on the same frames (the margin covers Farneback's float32 noise).  Measured on an MI355X: device 0.02542 /
    0.01277 / 0.03407 px-equivalents on steps of 1.5 / 2 / 1 px, the float64 chain the same to these digits."""
    frames, R_true, C_true = moving_camera()
    chain = chain_reference()
    st = Stabilizer(E2E_HW)
    R, Cm = st.rotations(frames)
    assert R.shape == (3, 3, 3) and Cm.shape == (4, 3, 3) and R.is_cuda and Cm.is_cuda and st.diag.shape == (3, 4)
    R, Cm = R.cpu().numpy(), Cm.cpu().numpy()
    W = E2E_HW[1]
    for t in range(3):
        e_dev, e_chain = sr.angle_between(R[t], R_true[t]), sr.angle_between(chain[t], R_true[t])
        step = sr.angle_between(R_true[t], np.eye(3))
        print('pair %d: step %.3f px, device error %.5f px, float64 chain error %.5f px' % (t, step * W / (2 * np.pi),
                                                                                          e_dev * W / (2 * np.pi), e_chain * W / (2 * np.pi)))
        assert e_dev <= 2 * e_chain
        assert e_chain <= 0.1 * step                     # the chain itself recovers the step
    np.testing.assert_allclose(Cm, sr.compose(R), atol=2e-7)
    assert np.array_equal(Cm[0], np.eye(3, dtype=np.float32))


def test_end_to_end_stabilised_video(tmp_path):
    """stabilize() brings the frames back to frame 0's orientation: their weighted frame-to-frame difference falls below the
    input's.  from_frames hands the stabilised video's flows to the training data path."""
    frames, _, _ = moving_camera()
    st = Stabilizer(E2E_HW)
    out, Cm = st.stabilize(frames)
    assert out.shape == frames.shape and out.dtype == torch.uint8 and out.is_cuda
    out = out.cpu().numpy()
    assert np.array_equal(out[0], frames[0])
    # the re-rendering itself is the resampler's: the restatement at the device's C
    want = sr.equirect_rotate(frames[1:], Cm[1:].cpu().numpy().astype(np.float64))
    assert np.max(np.abs(out[1:].astype(np.int32) - want.astype(np.int32))) <= 1
    before, after = weighted_frame_difference(frames), weighted_frame_difference(out)
    print('weighted mean |frame difference|: input %.3f, stabilised %.3f levels (ratio %.3f)' % (before, after, after / before))
    assert after < before
    flows = st.from_frames(frames)
    assert flows.shape == (3, 64, 128, 2) and flows.is_cuda and flows.dtype == torch.float32
    np.testing.assert_array_equal(flows.cpu().numpy(), st.flow.from_frames(out, res=(128, 64)).cpu().numpy())
    raw = st.flow.from_frames(frames, res=(128, 64))
    w = torch.from_numpy(sr.tables(64, 128, np.float32)[2]).to(DEV)[None, :, None, None]
    assert float((w * flows.abs()).mean()) < float((w * raw.abs()).mean())          # the camera's share is gone
    vd = tmp_path / 'videos' / 'clip_a'
    npy_io.save_motions(str(vd), flows)
    os.makedirs(str(vd / 'cube_feat'))
    for no in (2, 3, 4):
        np.save(npy_io.cube_feat_path(str(vd), no), np.full((6, 3, 2, 2), no, np.float32))
    lst = tmp_path / 'list.txt'
    lst.write_text('clip_a\n')
    ds = Sal360Dataset(str(tmp_path / 'videos'), str(tmp_path / 'videos'), str(lst), seq_len=2)
    assert len(ds) == 1
    seq, motion, category, filename = ds[0]
    assert category == 'clip_a' and filename == '000002.npy' and len(seq) == len(motion) == 2
    for t in range(2):
        assert motion[t].dtype == torch.float32 and tuple(motion[t].shape) == (64, 128, 2)
        np.testing.assert_array_equal(motion[t].numpy(), flows[t].cpu().numpy())
