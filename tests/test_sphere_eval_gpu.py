"""Sphere-weighted saliency metrics on the GPU (K14, csrc/sphere_eval.hip) against the numpy restatement of their specification
(tests/sphere_eval_restate.py, whose own claims tests/test_sphere_eval_cpu.py pins).

Tolerances.  The resampler is restated operation by operation in float32: bit-equal.  n_fix is an integer: exact.  The AUC is a
sum of at most 28 801 positive float64 terms <= 1 in the restatement, n eps = 3e-12: 1e-10 absolute, a 30-fold margin - and the
kernel's one quotient of integers equals the restatement's exact form bit for bit.  NSS, CC, SIM and KL are sums of at most
28 800 float64 terms, quotients of such sums and one log: 1e-9, relative or absolute.

Inputs (sphere_eval_restate.video: hash noise plus three von Mises-Fisher blobs of 12 degrees per ground-truth frame).  The
derived n_fix over both weight tables, checked here on the CPU: 5 - 12 at 8 x 16, 89 - 120 at 33 x 66, 932 - 2579 at 120 x 240;
never 0 or P."""
import functools
import math

import numpy as np
import pytest
import torch

from cp_360_weakly_supervised_saliency_amd import ops
from cp_360_weakly_supervised_saliency_amd.utils import eval_saliency, eval_sphere, hashrng, npy_io
from tests import sphere_eval_restate as rs

pytestmark = pytest.mark.gpu
DEV = 'cuda'
N_FIX_RANGE = {(8, 16): (5, 12), (33, 66): (89, 120), (120, 240): (932, 2579)}


def dev(a):
    return torch.from_numpy(np.array(a, order='C')).to(DEV)            # a copy: the shared inputs are read-only


def noise(seed, *shape):
    return hashrng.uniform(seed, shape, 0.0, 1.0, dtype=np.float64).astype(np.float32)


@functools.lru_cache(maxsize=None)
def clip(F, h, w):
    """(sal, gt) f32 [F, h, w] on the grid, read-only."""
    sal, gt = rs.video(1500 + h, F, h, w, h, w)
    sal.setflags(write=False)
    gt.setflags(write=False)
    return sal, gt


@functools.lru_cache(maxsize=None)
def restated(F, h, w, mode):
    """The restatement's (scores with the trapezoid AUC, scores with the exact AUC, n_fix) of clip(F, h, w), derived fixations."""
    sal, gt = clip(F, h, w)
    a = rs.weights(h, mode)
    want, n = rs.scores(sal, gt, a)
    return want, rs.scores(sal, gt, a, exact_auc=True)[0], n


def wt(h, mode='solid_angle'):
    return ops.sphere_eval_weights(h, mode, torch.device(DEV, torch.cuda.current_device()))


def assert_scores(got, want, exact=None):
    """got f64 [F, 5] (host) against the restatement's: the AUC within 1e-10, the rest within 1e-9 relative or absolute; NaN
    where the restatement has NaN."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.float64
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    for f in range(want.shape[0]):
        for k, name in enumerate(rs.NAMES):
            if math.isnan(want[f, k]):
                continue
            err = abs(got[f, k] - want[f, k])
            print('frame %d %s: %.15g against %.15g, apart %.2e' % (f, name, got[f, k], want[f, k], err))
            assert err <= (1e-10 if name == 'auc' else 1e-9 * max(1.0, abs(want[f, k]))), (f, name)
    if exact is not None:
        assert np.array_equal(got[:, 0], np.asarray(exact)[:, 0], equal_nan=True)


# ----------------------------------------------------------------------------- the resampler
@pytest.mark.parametrize('src_hw,hw', [((4, 8), (8, 16)), ((7, 14), (33, 66)), ((66, 132), (33, 66)), ((14, 28), (120, 240)),
                                       ((5, 9), (7, 30))])
def test_resample_is_bit_equal_to_the_restatement(src_hw, hw):
    src = noise(1510 + hw[0], 3, *src_hw)
    want = rs.resample(src, *hw)
    got = ops.sphere_eval_resample(dev(src), hw)
    assert got.shape == (3,) + hw and got.dtype == torch.float32 and got.is_cuda
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    # a [1:] view: frames that start 4 hs ws bytes into the allocation
    view = dev(src)[1:]
    assert view.is_contiguous()
    assert torch.equal(ops.sphere_eval_resample(view, hw).cpu(), torch.from_numpy(want[1:]))
    out = torch.empty((3,) + hw, dtype=torch.float32, device=DEV)
    assert ops.sphere_eval_resample(dev(src), hw, out=out) is out and torch.equal(out.cpu(), torch.from_numpy(want))


def test_resample_of_the_grids_own_size_is_a_bit_copy():
    src = noise(1520, 2, 33, 66)
    src[0, 0, :4] = (-0.0, np.inf, -np.inf, np.nan)
    src[1, 32, 65] = np.float32(1e-42)                                 # a subnormal
    got = ops.sphere_eval_resample(dev(src), (33, 66))
    assert got.data_ptr() != dev(src).data_ptr()
    assert torch.equal(got.cpu().view(torch.int32), torch.from_numpy(src).view(torch.int32))


# ----------------------------------------------------------------------------- scores against the restatement
@pytest.mark.parametrize('mode', ['solid_angle', 'uniform'])
@pytest.mark.parametrize('F,h,w', [(3, 8, 16), (3, 33, 66), (3, 120, 240)])
def test_scores_match_the_restatement(F, h, w, mode):
    """8 x 16: P = 128 is half a fixation tile and an eighth of a pixel tile; 33 x 66: P = 2178 is no multiple of 256 or 1024 and
    has an odd row count; 120 x 240: four to eleven fixation tiles and 29 pixel tiles per frame."""
    sal, gt = clip(F, h, w)
    want, exact, n = restated(F, h, w, mode)
    lo, hi = N_FIX_RANGE[(h, w)]
    assert all(lo <= v <= hi for v in n), n
    scores, n_fix = ops.sphere_eval(dev(sal), dev(gt), wt(h, mode))
    assert scores.shape == (F, 5) and scores.dtype == torch.float64 and scores.is_cuda
    assert n_fix.dtype == torch.int32 and n_fix.cpu().tolist() == n.tolist()
    assert_scores(scores.cpu().numpy(), want, exact)


def mask_of(n, h, w, seed=1530):
    """bool [h, w] with exactly n pixels set, scattered."""
    M = np.zeros(h * w, bool)
    M[np.argsort(hashrng.uniform(seed, (h * w,), dtype=np.float64), kind='stable')[:n]] = True
    return M.reshape(h, w)


@pytest.mark.parametrize('as_bool', [False, True])
def test_explicit_masks(as_bool):
    """33 x 66: one fixation; 600 (three fixation tiles, the last partly filled); all but one pixel (nine tiles); none and all
    (NaN AUC and NSS, the rest finite)."""
    h, w = 33, 66
    sal, gt = clip(3, h, w)
    counts = (1, 600, h * w - 1, 0, h * w)
    S = np.stack([sal[k % 3] for k in range(5)])
    G = np.stack([gt[k % 3] for k in range(5)])
    M = np.stack([mask_of(n, h, w) for n in counts])
    a = rs.weights(h)
    want, n = rs.scores(S, G, a, M)
    exact = rs.scores(S, G, a, M, exact_auc=True)[0]
    assert n.tolist() == list(counts)
    assert np.isnan(want[3:, :2]).all() and np.isfinite(want[3:, 2:]).all() and np.isfinite(want[:3]).all()
    fx = dev(M) if as_bool else dev(M.astype(np.uint8) * 7)           # any non-zero byte is a fixation
    scores, n_fix = ops.sphere_eval(dev(S), dev(G), wt(h), fixations=fx)
    assert n_fix.cpu().tolist() == list(counts)
    assert_scores(scores.cpu().numpy(), want, exact)


@pytest.mark.parametrize('mode', ['solid_angle', 'uniform'])
def test_quantised_maps(mode):
    """S on 8 levels: every level ties inside the mask, outside it and across it; tied fixations share a ROC point."""
    h, w = 33, 66
    S = (np.floor(noise(1540, 2, h, w) * 8.0) / 8.0).astype(np.float32)
    _, gt = clip(3, h, w)
    M = np.stack([noise(1541, h, w) > 0.9, mask_of(600, h, w, 1542)])
    for lvl in np.unique(S):
        assert all((S[f][M[f]] == lvl).sum() > 1 and (S[f][~M[f]] == lvl).sum() > 1 for f in range(2))
    a = rs.weights(h, mode)
    want, n = rs.scores(S, gt[:2], a, M)
    scores, n_fix = ops.sphere_eval(dev(S), dev(gt[:2]), wt(h, mode), fixations=dev(M))
    assert n_fix.cpu().tolist() == n.tolist()
    assert_scores(scores.cpu().numpy(), want, rs.scores(S, gt[:2], a, M, exact_auc=True)[0])
    # ... and with the derived mask, S = G quantised: the fixations are the top levels, all tied
    Gq = (np.floor(gt[:2] / gt[:2].max() * 8.0) / 8.0).astype(np.float32)
    want, n = rs.scores(Gq, Gq, a)
    assert all(0 < v < h * w for v in n)
    scores, n_fix = ops.sphere_eval(dev(Gq), dev(Gq), wt(h, mode))
    assert n_fix.cpu().tolist() == n.tolist()
    assert_scores(scores.cpu().numpy(), want, rs.scores(Gq, Gq, a, exact_auc=True)[0])


# ----------------------------------------------------------------------------- reproducibility
@pytest.mark.parametrize('h,w', [(33, 66), (120, 240)])
def test_batches_single_frames_and_places_are_bit_identical(h, w):
    sal, gt = clip(3, h, w)
    order = [0, 1, 2, 1, 0]                                            # frame 0 at places 0 and 4
    S, G = dev(np.stack([sal[k] for k in order])), dev(np.stack([gt[k] for k in order]))
    batch, n_batch = ops.sphere_eval(S, G, wt(h))
    again, _ = ops.sphere_eval(S, G, wt(h))
    assert torch.equal(batch, again)                                   # between runs (no NaN here: equal means bit-equal)
    assert not torch.isnan(batch).any()
    singles = [ops.sphere_eval(S[f:f + 1], G[f:f + 1], wt(h)) for f in range(5)]
    assert torch.equal(batch, torch.cat([s for s, _ in singles])) and torch.equal(n_batch, torch.cat([n for _, n in singles]))
    assert torch.equal(batch[0], batch[4]) and torch.equal(batch[1], batch[3])
    # a caller's workspace, larger than needed, with whatever an earlier call left in it
    work = ops.sphere_eval_work(8, h, w, S.device)
    work.fill_(float('nan'))
    assert torch.equal(ops.sphere_eval(S, G, wt(h), work=work)[0], batch)
    assert torch.equal(ops.sphere_eval(S[1:3], G[1:3], wt(h), work=work)[0], batch[1:3])


@pytest.mark.parametrize('bad', [float('nan'), float('inf')])
@pytest.mark.parametrize('which', ['S', 'G'])
def test_a_non_finite_frame_stays_alone(bad, which):
    h, w = 33, 66
    sal, gt = clip(3, h, w)
    clean, n_clean = ops.sphere_eval(dev(sal), dev(gt), wt(h))
    dirty = {'S': sal.copy(), 'G': gt.copy()}
    dirty[which][1, 17, 40] = bad
    scores, n_fix = ops.sphere_eval(dev(dirty['S']), dev(dirty['G']), wt(h))
    assert torch.isnan(scores[1]).all()
    assert torch.equal(scores[0], clean[0]) and torch.equal(scores[2], clean[2])
    assert n_fix[0] == n_clean[0] and n_fix[2] == n_clean[2]
    want, n = rs.scores(dirty['S'], dirty['G'], rs.weights(h))
    assert np.isnan(want[1]).all() and n_fix.cpu().tolist() == n.tolist()


def test_degenerate_frames():
    """No variance and no mass in S (CC, NSS, SIM, KL NaN; every fixation ties with every pixel: AUC 1/2), then in G."""
    h, w = 33, 66
    sal, gt = clip(3, h, w)
    flat = np.full((h, w), 0.5, np.float32)
    S, G = np.stack([flat, sal[1], sal[2]]), np.stack([gt[0], flat, gt[2]])
    a = rs.weights(h)
    want, n = rs.scores(S, G, a)
    assert np.isnan(want[0, 1:]).all() and want[0, 0] == 0.5 and np.isnan(want[1]).all() and n[1] == 0
    scores, n_fix = ops.sphere_eval(dev(S), dev(G), wt(h))
    assert n_fix.cpu().tolist() == n.tolist()
    assert_scores(scores.cpu().numpy(), want, rs.scores(S, G, a, exact_auc=True)[0])


# ----------------------------------------------------------------------------- K8 and the driver
def test_uniform_weights_agree_with_k8_on_its_own_grid():
    """120 x 240 maps: K8's resize is the identity, and a flat grid is the 'uniform' table."""
    sal, gt = clip(3, 120, 240)
    scores = ops.sphere_eval(dev(sal), dev(gt), wt(120, 'uniform'))[0].cpu().numpy()
    for f in range(2):
        s, g = sal[f].copy(), gt[f].copy()                             # the shared inputs are read-only
        cc, sim = eval_saliency.CorrCoeff(s, g), eval_saliency.similarity(s, g)
        print('frame %d: cc %.15g against K8 %.15g, sim %.15g against %.15g' % (f, scores[f, 2], cc, scores[f, 3], sim))
        assert abs(scores[f, 2] - cc) <= 1e-9 and abs(scores[f, 3] - sim) <= 1e-9


def test_sphere_eval_driver(tmp_path):
    """SphereEval on maps off the grid (14 x 28 predictions, 60 x 120 ground truth, three frames), its means, the dataset means
    and the file-based entry."""
    sal, gt = rs.video(1550, 3, 14, 28, 60, 120)
    ev = eval_sphere.SphereEval((33, 66))
    S, G = rs.resample(sal, 33, 66), rs.resample(gt, 33, 66)
    assert torch.equal(ev.resample(sal).cpu(), torch.from_numpy(S))
    want, n = rs.scores(S, G, rs.weights(33))
    r = ev.evaluate(sal, gt)
    assert len(r) == 3 and r.n_fix.cpu().tolist() == n.tolist() and r.frames is None
    assert_scores(r.scores.cpu().numpy(), want)
    for k, name in enumerate(eval_sphere.METRICS):
        field = getattr(r, name)
        assert field.is_cuda and field.dtype == torch.float64 and torch.equal(field, r.scores[:, k])
    assert torch.equal(ev.evaluate(dev(sal), dev(gt)).scores, r.scores)                # device maps, the workspace reused
    means = ev.means(r)
    for k, name in enumerate(eval_sphere.METRICS):
        assert abs(means[name] - want[:, k].mean()) <= 1e-9
    # explicit fixations on the grid; uniform weights
    M = np.stack([mask_of(40, 33, 66, 1551 + f) for f in range(3)])
    assert_scores(ev.evaluate(sal, gt, fixations=M).scores.cpu().numpy(), rs.scores(S, G, rs.weights(33), M)[0])
    flat = eval_sphere.SphereEval((33, 66), weights='uniform')
    assert_scores(flat.evaluate(sal, gt).scores.cpu().numpy(), rs.scores(S, G, rs.weights(33, 'uniform'))[0])
    # files: predictions 00004 .. 00006 of one video against <gt>/<video>.mp4/
    pred_dir, gt_dir = str(tmp_path / 'pred'), str(tmp_path / 'gt')
    for f, no in enumerate((4, 5, 6)):
        npy_io.save_saliency(pred_dir, 'vid', no, sal[f])
        npy_io.save_saliency(gt_dir, 'vid.mp4', no, gt[f])
    npy_io.save_saliency(gt_dir, 'vid.mp4', 7, gt[0])                  # ground truth without a prediction is not scored
    rf = eval_sphere.evaluate_video_dir(pred_dir, gt_dir, 'vid', ev)
    assert rf.frames == [4, 5, 6] and torch.equal(rf.scores, r.scores)
    second = dict(means, cc=means['cc'] - 0.5)
    whole = eval_sphere.dataset_means([means, second], [3, 9])
    assert abs(whole['cc'] - (means['cc'] - 0.375)) <= 1e-12 and abs(whole['auc_judd'] - means['auc_judd']) <= 1e-12
    npy_io.save_saliency(pred_dir, 'vid', 9, sal[0])
    with pytest.raises(FileNotFoundError):
        eval_sphere.evaluate_video_dir(pred_dir, gt_dir, 'vid', ev)


def test_errors():
    S = dev(clip(3, 8, 16)[0])
    w8 = wt(8)
    with pytest.raises(ValueError):
        ops.sphere_eval(S[0], S[0], w8)                                # no frame axis
    with pytest.raises(ValueError):
        ops.sphere_eval(S.double(), S.double(), w8)                    # wrong dtype
    with pytest.raises(ValueError):
        ops.sphere_eval(S[:, :, ::2], S[:, :, ::2], w8)                # not contiguous
    with pytest.raises(ValueError):
        ops.sphere_eval(S, S[:2], w8)                                  # another batch
    with pytest.raises(ValueError):
        ops.sphere_eval(S, S, wt(9))                                   # another geometry's table
    with pytest.raises(ValueError):
        ops.sphere_eval(S, S, w8.long())
    with pytest.raises(ValueError):
        ops.sphere_eval(S, S, w8, fixations=torch.zeros(3, 8, 16, device=DEV))         # float fixations
    with pytest.raises(ValueError):
        ops.sphere_eval(S, S, w8, fixations=torch.zeros(3, 8, 8, dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.sphere_eval(S, S.cpu(), w8)
    with pytest.raises(ValueError):
        ops.sphere_eval_resample(S[0], (8, 16))
    with pytest.raises(ValueError):
        ops.sphere_eval_resample(S.half(), (8, 16))
    with pytest.raises(ValueError):
        ops.sphere_eval_resample(S, (0, 16))
    with pytest.raises(ValueError):
        ops.sphere_eval_resample(S, (8, 16), out=torch.empty(3, 8, 8, device=DEV))
