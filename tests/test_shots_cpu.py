"""Shot detection (K13) without a GPU: the library's exports, host weight table and status codes, the claims of the integer
restatement (tests/shots_restate.py) that tests/test_shots_gpu.py holds the kernel to - the signature is invariant under a yaw
rotation, nearly so under any rotation, and jumps between scenes of different tone -, the cut decision (utils/shots.py against
the restatement and hand-made sequences) and the consumers' ``cuts=`` arguments (utils/stabilize.compose, utils/viewport.
smooth_path and cameras): per-shot results bit for bit, today's results without cuts, ValueError on bad cuts.

No test depends on ShotDetector's defaults: thr, ratio and radius are passed."""
import ctypes as C

import numpy as np
import pytest
import torch

from cp_360_weakly_supervised_saliency_amd import _lib, ops
from cp_360_weakly_supervised_saliency_amd.utils import hashrng
from cp_360_weakly_supervised_saliency_amd.utils import shots
from cp_360_weakly_supervised_saliency_amd.utils import stabilize as stab
from cp_360_weakly_supervised_saliency_amd.utils import viewport as vp
from tests import shots_restate as rs
from tests import stabilize_restate as sr

K13 = ('cp360_shot_weights_host', 'cp360_shot_work_bytes', 'cp360_shot_signatures')
NULL, BAD_SHAPE, ALIGN, UNSUPPORTED = -5, -1, -6, -8
THR, RATIO, RADIUS = 0.25, 3, 8


# ----------------------------------------------------------------------------- library
def test_library_exports_the_symbols():
    L = _lib.lib()
    for name in K13:
        assert name in _lib.PUBLIC_SYMBOLS and hasattr(L, name)


@pytest.mark.parametrize('H', [1, 2, 8, 33, 64, 480, 1024, 2048])
def test_host_weights(H):
    a, total = ops.shot_weights_host(H)
    want, want_total = rs.weights(H)
    assert a.dtype == np.int32 and a.shape == (H,)
    assert np.array_equal(a, want) and total == want_total == int(a.sum())
    assert np.array_equal(a, a[::-1])                                  # symmetric top to bottom
    assert a.min() >= 0 and a.max() <= 1024 and a[H // 2] == a.max()


def test_status_codes_without_gpu():
    """Argument validation happens before any launch: the dummy pointers are never used."""
    L = _lib.lib()
    one, big = C.c_void_p(16), 1 << 30
    buf = (C.c_int32 * 4)()
    assert L.cp360_shot_weights_host(4, None, None) == NULL
    assert L.cp360_shot_weights_host(0, C.cast(buf, C.c_void_p), None) == BAD_SHAPE
    assert L.cp360_shot_weights_host(4, C.cast(buf, C.c_void_p), None) == 0          # the total is optional
    sigs = lambda fr, F, H, W, wt, sg, wk, nb: L.cp360_shot_signatures(fr, F, H, W, wt, sg, wk, nb, None)
    ok = (one, 2, 16, 32, one, one, one, big)
    for k in (0, 4, 5, 6):
        args = list(ok)
        args[k] = None
        assert sigs(*args) == NULL
    for F, H, W in ((0, 16, 32), (2, 0, 32), (2, 16, 0), (-1, 16, 32), (2, -16, 32), (2, 16, -32)):
        assert sigs(one, F, H, W, one, one, one, big) == BAD_SHAPE
        assert L.cp360_shot_work_bytes(F, H, W) == 0
    assert sigs(one, 70000, 16, 32, one, one, one, big) == UNSUPPORTED                # grid y
    assert sigs(one, 1, 70000, 32, one, one, one, big) == UNSUPPORTED
    assert sigs(one, 1, 2, (1 << 21) + 1, one, one, one, big) == UNSUPPORTED           # a row's u32 partial
    assert sigs(one, 1, 1 << 30, 1 << 30, one, one, one, big) == UNSUPPORTED           # T >= 2^62
    assert L.cp360_shot_work_bytes(1, 1 << 30, 1 << 30) == 0
    need = L.cp360_shot_work_bytes(2, 16, 32)
    assert need > 0 and need % 16 == 0
    assert sigs(one, 2, 16, 32, one, one, one, need - 1) == BAD_SHAPE                 # workspace too small
    assert sigs(one, 2, 16, 32, one, one, C.c_void_p(8), big) == ALIGN
    assert sigs(one, 2, 16, 32, one, C.c_void_p(4), one, big) == ALIGN
    # u32 partial sums hold: a workgroup's rows times the width times the largest weight stays below 2^32 (W = 2^21: one row)
    for F, H, W in ((1, 480, 960), (64, 2048, 4096), (1, 8, 1 << 21), (3, 33, 66)):
        nblk = L.cp360_shot_work_bytes(F, H, W) // (192 * 4) // F
        rows = -(-H // nblk)
        assert nblk >= 1 and rows * W * 1024 < 2 ** 32, (F, H, W, nblk)


# (F, H, W) -> R: both sides of the switch to 16 rows (F ceil(H / 16) = 1024 | 1008 | 1023), and of every halving for wide rows
ROW_RULE = [((64, 250, 22), 16), ((63, 250, 22), 8), ((1, 5, 262145), 4), ((1, 3, 1048577), 1),
            ((64, 256, 22), 16), ((1023, 16, 8), 8), ((1024, 16, 8), 16), ((1024, 1, 8), 16), ((2, 480, 960), 8),
            ((16, 960, 1920), 8), ((18, 960, 1920), 16), ((1024, 16, 131072), 16), ((1024, 16, 131073), 8),
            ((1, 5, 262144), 8), ((1, 5, 524288), 4), ((1, 5, 524289), 2), ((1, 3, 1048576), 2), ((1, 3, 1 << 21), 1),
            ((1024, 16, 1 << 21), 1), ((3, 33, 66), 8), ((3, 8, 16), 8)]


@pytest.mark.parametrize('shape,R', ROW_RULE)
def test_work_bytes_prove_the_rows_per_workgroup(shape, R):
    """shot_rows() of csrc/shots.hip, restated in tests/shots_restate.py and held to the library without a launch: the workspace
    is F ceil(H / R) partial histograms, so its size tells R wherever ceil(H / R) differs between the candidates."""
    F, H, W = shape
    assert rs.shot_rows(F, H, W) == R
    assert _lib.lib().cp360_shot_work_bytes(F, H, W) == rs.work_bytes(F, H, W) == -(-(F * -(-H // R) * 768) // 16) * 16
    if shape in ROW_RULE[:4]:                                          # the shapes tests/test_shots_gpu.py launches
        assert all(-(-H // r) != -(-H // R) for r in (1, 2, 4, 8, 16) if r != R)


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.shot_signatures(torch.zeros(2, 8, 16, 3, dtype=torch.uint8))
    with pytest.raises(ValueError):
        ops.shot_weights_host(0)
    with pytest.raises(ValueError):
        ops.shot_distances(torch.zeros(2, 3, 64))                      # not int64
    with pytest.raises(ValueError):
        ops.shot_distances(torch.zeros(3, 64, dtype=torch.int64))
    with pytest.raises(ValueError):
        shots.ShotDetector(thr=1.5, ratio=3, radius=8, device='cpu')
    with pytest.raises(ValueError):
        shots.ShotDetector(thr=0.25, ratio=3, radius=-1, device='cpu')


def test_distances_in_torch_match_the_restatement():
    """ops.shot_distances is plain torch integer arithmetic: it runs on the restatement's signatures here."""
    sig, T = rs.signatures(rs.three_shot_video(32, 64))
    sad, Tt = ops.shot_distances(torch.from_numpy(sig))
    assert sad.dtype == torch.int64 and np.array_equal(sad.numpy(), rs.sad(sig)) and int(Tt) == T
    one, _ = ops.shot_distances(torch.from_numpy(sig[:1]))
    assert tuple(one.shape) == (0,)


# ----------------------------------------------------------------------------- the restatement's own claims
@pytest.mark.parametrize('hw', [(8, 16), (33, 66), (64, 128)])
def test_every_channel_sums_to_T(hw):
    frames = np.stack([rs.scene(k, *hw) for k in range(3)])
    sig, T = rs.signatures(frames)
    assert T == hw[1] * rs.weights(hw[0])[1]
    assert np.all(sig.sum(axis=2) == T) and sig.min() >= 0
    d = rs.distances(frames)
    assert np.all(d >= 0.0) and np.all(d <= 1.0)
    # two frames with no bin in common are at distance 1
    far = np.stack([np.zeros(hw + (3,), np.uint8), np.full(hw + (3,), 255, np.uint8)])
    assert rs.distances(far)[0] == 1.0


def test_yaw_is_a_column_roll_and_leaves_the_signature_alone():
    frame = rs.scene(0, 33, 66)
    want = rs.signatures(frame[None])[0]
    for k in (1, 7, 33, 65):
        assert np.array_equal(rs.signatures(np.roll(frame, k, axis=1)[None])[0], want)


def test_rotations_are_quiet_and_tones_are_loud():
    """64 x 128: a scene against itself rotated by 3, 15 and 90 degrees about three axes has d <= 0.1 (measured: at most
    0.0399); two scenes of different tone have d >= 0.4 (measured: 0.5533, 0.5995, 0.7825)."""
    H, W = 64, 128
    worst = 0.0
    for k in range(3):
        s = rs.scene(k, H, W)
        for axis in (sr.AXIS, (1.0, 0.0, 0.0), (0.0, 0.0, 1.0)):
            for deg in (3.0, 15.0, 90.0):
                turned = sr.equirect_rotate(s[None], sr.rot(axis, np.deg2rad(deg))[None])[0]
                worst = max(worst, float(rs.distances(np.stack([s, turned]))[0]))
    print('largest d under a rotation: %.4f' % worst)
    assert worst <= 0.1
    for i, j in ((0, 1), (0, 2), (1, 2)):
        d = float(rs.distances(np.stack([rs.scene(i, H, W), rs.scene(j, H, W)]))[0])
        print('scenes %d, %d: d = %.4f' % (i, j, d))
        assert d >= 0.4


# ----------------------------------------------------------------------------- find_cuts, segments
SEQUENCES = [
    ([0.02, 0.03, 0.6, 0.02, 0.04, 0.03], [3]),                        # an isolated peak
    ([0.02, 0.03, 0.6, 0.7, 0.04, 0.03, 0.02], [3, 4]),                # two adjacent peaks: a one-frame shot
    ([0.02, 0.03, 0.2, 0.02, 0.04], []),                               # a peak below thr
    ([0.2, 0.3, 0.5, 0.25, 0.3, 0.2], []),                             # above thr, below ratio * median (0.25)
    ([0.9], [1]),                                                      # F - 1 = 1: no neighbours, the median is 0
    ([0.1], []),
    ([], []),                                                          # one frame
    ([0.25, 0.0, 0.0], [1]),                                           # d = thr counts, at the first pair
    ([0.0, 0.0, 0.3], [3]),                                            # ... and at the last
]


@pytest.mark.parametrize('d,want', SEQUENCES)
def test_find_cuts_on_hand_made_sequences(d, want):
    assert shots.find_cuts(d, THR, RATIO, RADIUS) == want
    assert rs.find_cuts(d, THR, RATIO, RADIUS) == want


def test_find_cuts_window_and_parity():
    # the window: with radius 1 the busy stretch further away does not count, with radius 8 it raises the median
    d = [0.3, 0.3, 0.3, 0.3, 0.02, 0.5, 0.02, 0.3, 0.3, 0.3, 0.3]
    assert shots.find_cuts(d, THR, RATIO, 1) == [6] == rs.find_cuts(d, THR, RATIO, 1)
    assert shots.find_cuts(d, THR, RATIO, 8) == [] == rs.find_cuts(d, THR, RATIO, 8)
    assert shots.find_cuts(d, THR, RATIO, 0) == [i + 1 for i, v in enumerate(d) if v >= THR]
    for seed in range(6):
        d = hashrng.uniform(950 + seed, (40,), 0.0, 1.0).astype(np.float64) ** 3
        for thr, ratio, radius in ((0.25, 3, 8), (0.1, 1.5, 2), (0.0, 0.0, 3), (0.5, 10, 40)):
            assert shots.find_cuts(d, thr, ratio, radius) == rs.find_cuts(d, thr, ratio, radius)
    with pytest.raises(ValueError):
        shots.find_cuts([0.1], THR, RATIO, -1)


def test_segments_round_trip():
    for cuts, n in (([], 1), ([], 7), ([3], 7), ([1, 2, 6], 7), ([5, 6], 10)):
        seg = shots.segments(cuts, n)
        assert seg == rs.segments(cuts, n)
        assert seg[0][0] == 0 and seg[-1][1] == n and all(a[1] == b[0] for a, b in zip(seg[:-1], seg[1:]))
        assert all(hi > lo for lo, hi in seg) and [lo for lo, _ in seg[1:]] == cuts
    assert shots.segments(None, 4) == [(0, 4)]


BAD_CUTS = [([0], 5), ([5], 5), ([2, 2], 5), ([3, 2], 5), ([-1], 5), ([1.5], 5), ([True], 5), (['2'], 5), ([1], 1)]


@pytest.mark.parametrize('cuts,n', BAD_CUTS)
def test_bad_cuts_raise(cuts, n):
    with pytest.raises(ValueError):
        shots.check_cuts(cuts, n)
    with pytest.raises(ValueError):
        shots.segments(cuts, n)
    with pytest.raises(ValueError):
        stab.compose(np.stack([np.eye(3)] * (n - 1)) if n > 1 else np.zeros((0, 3, 3)), cuts)
    path = hashrng.normal(960, (n, 3), dtype=np.float64)
    with pytest.raises(ValueError):
        vp.smooth_path(path, 0.85, None, cuts)
    with pytest.raises(ValueError):
        vp.cameras(path, cuts)


def test_numpy_integers_are_cuts():
    assert shots.check_cuts(np.array([2, 4]), 6) == [2, 4] and shots.check_cuts((np.int64(1),), 3) == [1]


# ----------------------------------------------------------------------------- the three-shot video
@pytest.mark.parametrize('hw', [(32, 64), (33, 66), (64, 128)])
def test_three_shot_video(hw):
    """Shots of 5, 1 and 4 frames, each scene turning 4 degrees per frame about (0.3, 0.8, -0.52).  Measured: within a shot
    d <= 0.0633 (32 x 64), 0.0621 (33 x 66), 0.0373 (64 x 128); across the two cuts d >= 0.5849, 0.4692, 0.5533."""
    d = rs.distances(rs.three_shot_video(*hw))
    assert d.shape == (9,) and d.dtype == np.float64
    inside = max(d[t] for t in range(9) if t not in (4, 5))
    print('%s: within a shot d <= %.4f, across the cuts d >= %.4f' % (hw, inside, min(d[4], d[5])))
    assert rs.find_cuts(d, THR, RATIO, RADIUS) == rs.THREE_SHOT_CUTS
    assert shots.find_cuts(d, THR, RATIO, RADIUS) == rs.THREE_SHOT_CUTS
    assert shots.segments(rs.THREE_SHOT_CUTS, 10) == [(0, 5), (5, 6), (6, 10)]


# ----------------------------------------------------------------------------- consumers
def some_rotations(n, seed):
    axes = hashrng.normal(seed, (n, 3), dtype=np.float64)
    return np.stack([sr.rot(a, 0.05 * (i + 1)) for i, a in enumerate(axes)]).astype(np.float32)


@pytest.mark.parametrize('cuts', [[5, 6], [1], [9], [1, 2, 3], [4]])
def test_compose_restarts_at_every_cut(cuts):
    R = some_rotations(9, 970)
    C = stab.compose(R, cuts)
    assert C.shape == (10, 3, 3) and C.dtype == np.float64
    for lo, hi in shots.segments(cuts, 10):
        assert np.array_equal(C[lo], np.eye(3))
        assert np.array_equal(C[lo:hi], stab.compose(R[lo:hi - 1]))    # the shot's own pairs; the straddling R is not used
    # ... whatever the straddling pair's R holds
    R2 = R.copy()
    R2[[c - 1 for c in cuts]] = np.nan
    assert np.array_equal(stab.compose(R2, cuts), C)


def test_compose_without_cuts_is_unchanged():
    R = some_rotations(9, 971)
    want = sr.compose(R)                                               # the restatement of the chain as it was
    assert np.array_equal(stab.compose(R), want) and np.array_equal(stab.compose(R, None), want)
    assert np.array_equal(stab.compose(R, []), want)


def noisy_path(n, seed):
    t = np.linspace(0.0, 3.0, n)
    c = np.stack([np.cos(t) * np.cos(0.4 * t), np.sin(0.4 * t), np.sin(t) * np.cos(0.4 * t)], 1)
    c = c + 0.15 * hashrng.normal(seed, c.shape, dtype=np.float64)
    c[3] = (0.0, 1.0, 0.0)                                             # a pole: look_at takes the previous frame's right there
    c[6] = (0.0, -1.0, 0.0)
    return c


@pytest.mark.parametrize('cuts', [[5, 6], [1], [9], [3], [6], [2, 3, 4]])
@pytest.mark.parametrize('alpha,max_step', [(0.85, None), (0.5, 3.0)])
def test_smooth_path_and_cameras_run_shot_by_shot(cuts, alpha, max_step):
    c = noisy_path(10, 980)
    got = vp.smooth_path(c, alpha, max_step, cuts)
    want = np.concatenate([vp.smooth_path(c[lo:hi], alpha, max_step) for lo, hi in shots.segments(cuts, 10)])
    assert got.shape == (10, 3) and np.array_equal(got, want)
    cams = vp.cameras(c, cuts)
    want_cams = np.concatenate([vp.cameras(c[lo:hi]) for lo, hi in shots.segments(cuts, 10)])
    assert cams.shape == (10, 3, 3) and np.array_equal(cams, want_cams)


def test_smooth_path_and_cameras_without_cuts_are_unchanged():
    from tests import viewport_restate as vr
    c = noisy_path(10, 981)
    for alpha, max_step in ((0.85, None), (0.5, 3.0)):
        base = vp.smooth_path(c, alpha, max_step)
        assert np.array_equal(vp.smooth_path(c, alpha, max_step, None), base) and np.array_equal(vp.smooth_path(c, alpha, max_step, []), base)
        assert np.max(np.abs(base - vr.smooth_path(c, alpha, max_step))) < 1e-12
    assert np.array_equal(vp.cameras(c, None), vp.cameras(c)) and np.array_equal(vp.cameras(c, []), vp.cameras(c))
    assert np.max(np.abs(vp.cameras(c) - vr.cameras(c))) < 1e-12
    # the cut matters: the camera of a shot's first frame at a pole does not inherit the previous scene's right
    assert not np.array_equal(vp.cameras(c, [3]), vp.cameras(c))
    assert not np.array_equal(vp.smooth_path(c, 0.85, None, [5]), vp.smooth_path(c, 0.85))
