"""Fixation maps and shuffled AUC on the GPU (K15, csrc/fixations.hip) against the numpy restatement of their specification
(tests/fixations_restate.py, whose own claims tests/test_fixations_cpu.py pins).

Tolerances.  Counts, n_points, c_tot and a_neg are integers: equal.  The shuffled AUC is one quotient of integers below 2^53,
rounded once: bit-equal to the restatement's quotient of Python integers.  The density is a float32 sum of expf terms: held to
the float64 definition within DENSITY_GATE[sigma] of the frame's maximum (below).  Batch and workspace independence: torch.equal.

Inputs: frames of 64, 0, 1, 300 and a handful of points (300 crosses the 256-point LDS tile of the density kernel and the
256-thread stride of the counts kernel), on 8 x 16 (one workgroup), 33 x 66 (9 workgroups, P no multiple of 256) and 120 x 240."""
import functools
import math

import numpy as np
import pytest
import torch

from cp_360_weakly_supervised_saliency_amd import ops
from cp_360_weakly_supervised_saliency_amd.utils import eval_sphere, fixations, hashrng, npy_io
from tests import fixations_restate as fr

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GRIDS = [(8, 16), (33, 66), (120, 240)]
SIGMAS_DEG = [2.0, 5.0, 20.0]
# The largest pixel-wise error of a density map against the float64 definition, in units of the frame's maximum, over the three
# grids and the five frames below, per sigma.  The error is the float32 rounding of the dot product (2^-24 near 1) times kappa =
# 1 / sigma^2 (821, 131, 8.2), carried through the exponential: it falls with sigma, so every sigma has its own gate.  Measured
# (float32 restatement on the CPU = density32, the kernel's operations in its order; the kernel on an MI355X):
DENSITY_MEASURED = {2.0: (6.889e-5, 6.895e-5), 5.0: (1.491e-5, 1.491e-5), 20.0: (1.202e-6, 1.259e-6)}
# The gate is four times the larger of the two: expf and the rounding of q may differ by a few ulp between the device and numpy,
# and four leaves room for that without hiding a wrong kernel (a dropped or doubled point moves a pixel by up to 1 / 300 of the
# maximum or more, an operation out of order in the dot product by about as much as the measured error itself).
DENSITY_GATE = {s: 4.0 * max(m) for s, m in DENSITY_MEASURED.items()}


def dev(a):
    return torch.from_numpy(np.array(a, order='C')).to(DEV)            # a copy: the shared inputs are read-only


@functools.lru_cache(maxsize=None)
def density_points():
    """(lonlat, offsets) of 5 frames: 64, 0, 1 and 300 random points and a frame of special ones (two that are dropped, two
    beyond the range, one on the pole)."""
    lonlat, offsets = fr.random_points(1801, [64, 0, 1, 300])
    special = np.array([[np.nan, 0.1], [0.3, np.inf], [0.3, 2.0], [-4.0, -0.2], [1.0, np.pi / 2.0]])
    lonlat = np.ascontiguousarray(np.concatenate([lonlat, special]))
    offsets = np.concatenate([offsets, [offsets[-1] + len(special)]]).astype(np.int32)
    lonlat.setflags(write=False)
    offsets.setflags(write=False)
    return lonlat, offsets


@functools.lru_cache(maxsize=None)
def count_points(h, w):
    """5 frames: 64 random points, none, one, 300, and the edges of the binning with 40 more points in one pixel."""
    lonlat, offsets = fr.random_points(1802, [64, 0, 1, 300])
    edges = fr.edge_points(h, w)[0]
    lonlat = np.ascontiguousarray(np.concatenate([lonlat, edges, np.tile([[0.5, 0.25]], (40, 1))]))
    offsets = np.concatenate([offsets, [len(lonlat)]]).astype(np.int32)
    lonlat.setflags(write=False)
    offsets.setflags(write=False)
    return lonlat, offsets


@functools.lru_cache(maxsize=None)
def restated_density(h, w, sigma_deg):
    lonlat, offsets = density_points()
    G = fr.density64(lonlat, offsets, h, w, np.deg2rad(sigma_deg))
    G.setflags(write=False)
    return G


def density_error(got, want):
    """The largest |got - want| of every frame in units of the frame's maximum (frames of zeros: absolute)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    peak = want.reshape(len(want), -1).max(axis=1)
    return float(np.max(np.abs(got - want).reshape(len(want), -1).max(axis=1) / np.where(peak > 0.0, peak, 1.0)))


# ----------------------------------------------------------------------------- counts
@pytest.mark.parametrize('hw', GRIDS)
def test_counts_equal_the_restatement(hw):
    lonlat, offsets = count_points(*hw)
    want, want_n = fr.bin_points(lonlat, offsets, *hw)
    counts, n = ops.fixation_counts(dev(lonlat), dev(offsets), hw)
    assert counts.dtype == torch.int32 and n.dtype == torch.int32 and tuple(counts.shape) == (5,) + hw
    assert torch.equal(counts.cpu().long(), torch.from_numpy(want)) and torch.equal(n.cpu().long(), torch.from_numpy(want_n))
    assert want_n.tolist()[:4] == [64, 0, 1, 300] and int(want[4].max()) >= 40 and int(want[1].sum()) == 0
    assert int(want_n[4]) == offsets[5] - offsets[4] - 5                # the five non-finite points are not counted


def test_counts_without_points_and_with_offsets_out_of_range():
    empty = torch.zeros((0, 2), dtype=torch.float64, device=DEV)
    counts, n = ops.fixation_counts(empty, dev(np.zeros(4, np.int32)), (8, 16))
    assert not counts.any() and not n.any() and tuple(counts.shape) == (3, 8, 16)
    lonlat, _ = fr.random_points(1803, [10])
    counts, n = ops.fixation_counts(dev(lonlat), dev(np.array([-5, 4, 99], np.int32)), (8, 16))       # clamped into 0 .. N
    want, want_n = fr.bin_points(lonlat, [0, 4, 10], 8, 16)
    assert torch.equal(counts.cpu().long(), torch.from_numpy(want)) and n.tolist() == want_n.tolist()


# ----------------------------------------------------------------------------- density
@pytest.mark.parametrize('sigma_deg', SIGMAS_DEG)
@pytest.mark.parametrize('hw', GRIDS)
def test_density_against_the_float64_definition(hw, sigma_deg):
    lonlat, offsets = density_points()
    want = restated_density(*hw, sigma_deg)
    cpu = density_error(fr.density32(lonlat, offsets, *hw, np.deg2rad(sigma_deg)), want)
    G = ops.fixation_density(dev(lonlat), dev(offsets), hw, np.deg2rad(sigma_deg))
    assert G.dtype == torch.float32 and tuple(G.shape) == (5,) + hw
    got = G.cpu().numpy()
    gpu = density_error(got, want)
    print('density %s sigma %g: float32 restatement %.3e, kernel %.3e of the maximum (gate %.3e)' % (hw, sigma_deg, cpu, gpu, DENSITY_GATE[sigma_deg]))
    assert cpu <= DENSITY_GATE[sigma_deg] and gpu <= DENSITY_GATE[sigma_deg]
    assert not got[1].any() and got[4].max() > 0.0                     # no points: exactly zero; dropped points leave the rest


def test_density_does_not_depend_on_the_batch_or_the_place():
    hw, sigma = (33, 66), np.deg2rad(5.0)
    lonlat, offsets = density_points()
    batch = ops.fixation_density(dev(lonlat), dev(offsets), hw, sigma)
    for f in range(5):
        one = ops.fixation_density(dev(lonlat[offsets[f]:offsets[f + 1]]), dev(np.array([0, offsets[f + 1] - offsets[f]], np.int32)), hw, sigma)
        assert torch.equal(one[0], batch[f]), f
    p3 = lonlat[offsets[3]:offsets[4]]                                  # the 300-point frame at places 0 and 4
    again = np.concatenate([p3, lonlat[offsets[0]:offsets[3]], p3])
    offs = np.array([0, 300, 364, 364, 365, 665], np.int32)
    moved = ops.fixation_density(dev(again), dev(offs), hw, sigma)
    assert torch.equal(moved[0], batch[3]) and torch.equal(moved[4], batch[3]) and torch.equal(moved[1], batch[0])


def test_a_workspace_full_of_nan_changes_nothing():
    hw, sigma = (33, 66), np.deg2rad(5.0)
    lonlat, offsets = density_points()
    nan_work = lambda F: torch.full_like(ops.fixation_work(F, *hw, torch.device(DEV, torch.cuda.current_device())), float('nan'))
    a = ops.fixation_density(dev(lonlat), dev(offsets), hw, sigma)
    b = ops.fixation_density(dev(lonlat), dev(offsets), hw, sigma, work=nan_work(0))
    assert torch.equal(a, b)
    S, pos, neg = sauc_inputs(hw)
    want = ops.shuffled_auc(dev(S), dev(pos), dev(neg))
    got = ops.shuffled_auc(dev(S), dev(pos), dev(neg), work=nan_work(len(S)))
    assert all(torch.equal(x, y) for x, y in zip(want, got)) and not torch.isnan(got[0]).any()


# ----------------------------------------------------------------------------- shuffled AUC
@functools.lru_cache(maxsize=None)
def sauc_inputs(hw, levels=None):
    """(S f32 [4, h, w], pos int32 [4, h, w], neg int32 [4, h, w]): the counts of count_points' first four frames (64, 0, 1, 300
    points) with frame 1 given frame 3's, the negatives the other frames' counts."""
    h, w = hw
    lonlat, offsets = count_points(h, w)
    counts = fr.bin_points(lonlat, offsets, h, w)[0][:4]
    counts[1] = counts[3]
    S = fr.quantised(1810 + h, 4, h, w, levels) if levels else hashrng.uniform(1810 + h, (4, h, w), 0.0, 1.0, dtype=np.float64).astype(np.float32)
    S[0] += counts[0].astype(np.float32)                               # frame 0 knows its fixations: a high score
    out = S, counts.astype(np.int32), fr.other_frames(counts).astype(np.int32)
    for a in out:
        a.setflags(write=False)
    return out


def assert_sauc(got, S, pos, neg):
    auc, c_tot, a_neg = (t.cpu().numpy() for t in got)
    want, want_c, want_a = fr.sauc_video(S, pos, neg)
    assert auc.dtype == np.float64 and c_tot.dtype == np.int64 and a_neg.dtype == np.int64
    print('sAUC', auc.tolist(), 'restated', want.tolist())
    assert np.array_equal(c_tot, want_c) and np.array_equal(a_neg, want_a)
    assert np.array_equal(auc, want, equal_nan=True)                   # bit for bit
    return auc


@pytest.mark.parametrize('levels', [None, 8])
@pytest.mark.parametrize('hw', GRIDS)
def test_sauc_is_bit_equal_to_the_exact_quotient(hw, levels):
    S, pos, neg = sauc_inputs(hw, levels)
    auc = assert_sauc(ops.shuffled_auc(dev(S), dev(pos), dev(neg)), S, pos, neg)
    assert not np.isnan(auc).any() and auc[0] > auc[1:].max()        # frame 0's map knows its fixations, the others are noise
    one_map = pos.sum(axis=0, keepdims=True).astype(np.int32)          # a dataset-wide negative map: [1, h, w]
    got = ops.shuffled_auc(dev(S), dev(pos), dev(one_map))
    assert_sauc(got, S, pos, one_map)
    same = ops.shuffled_auc(dev(S), dev(pos), dev(np.repeat(one_map, 4, axis=0)))
    assert all(torch.equal(x, y) for x, y in zip(got, same))


def test_sauc_multiplicities_and_clamps():
    h, w = 33, 66
    S, pos, neg = (a.copy() for a in sauc_inputs((h, w), 8))
    pos[0, 3, 4:9] = [1023, 1024, 5000, -7, 1]                         # at the clamp, above it, below zero
    neg[0, 5, 0:5] = [1 << 20, (1 << 20) + 5, 1 << 30, -1, 0]
    neg[2] = [[1 << 20]]                                               # 2 A_neg C_tot = 2 * 2178 * 2^20 * 1 < 2^53
    auc = assert_sauc(ops.shuffled_auc(dev(S), dev(pos), dev(neg)), S, pos, neg)
    assert not np.isnan(auc).any()
    pos[:] = 1023
    neg[:] = 1 << 20
    assert 2 * (h * w * 1023) * (h * w << 20) >= 1 << 53               # every frame: beyond the exact range
    auc = assert_sauc(ops.shuffled_auc(dev(S), dev(pos), dev(neg)), S, pos, neg)
    assert np.isnan(auc).all()


def test_sauc_degenerate_frames_and_exact_halves():
    hw = (33, 66)
    S, pos, neg = (a.copy() for a in sauc_inputs(hw))
    S[1, 7, 7] = np.nan                                                # a NaN in frame 1: that frame only
    pos[2] = 0                                                         # C_tot = 0
    neg[3] = 0                                                         # A_neg = 0
    auc = assert_sauc(ops.shuffled_auc(dev(S), dev(pos), dev(neg)), S, pos, neg)
    assert np.isnan(auc).tolist() == [False, True, True, True]
    S, pos, neg = (a.copy() for a in sauc_inputs(hw))
    S[1] = 0.375                                                       # a constant map
    neg[2] = pos[2]                                                    # negatives = positives
    S[3] = np.inf                                                      # constant, but not finite
    auc = assert_sauc(ops.shuffled_auc(dev(S), dev(pos), dev(neg)), S, pos, neg)
    assert auc[1] == 0.5 and auc[2] == 0.5 and math.isnan(auc[3])


@pytest.mark.parametrize('hw', [(8, 16), (33, 66)])
def test_auc_judd_and_shuffled_auc_are_one_engine(hw):
    """K14's AUC-Judd of a mask M is K15's shuffled AUC with pos = M and neg = a (1 - M): K14's packed-word kernels and K15's
    sum by parts give the same bits.  Frame 0 is continuous, frame 1 quantised (ties inside and across the mask), frame
    2 has an empty mask: the NaN of both."""
    h, w = hw
    S = hashrng.uniform(1880 + h, (3, h, w), 0.0, 1.0, dtype=np.float64).astype(np.float32)
    S[1] = fr.quantised(1881 + h, 1, h, w, 8)[0]
    M = hashrng.uniform(1882 + h, (3, h, w), 0.0, 1.0, dtype=np.float64) > 0.6
    M[2] = False
    assert set(S[1][M[1]].tolist()) == set(S[1][~M[1]].tolist()) and len(set(S[1][M[1]].tolist())) == 8 < M[1].sum() // 4
    G = hashrng.uniform(1883 + h, (3, h, w), 0.0, 1.0, dtype=np.float64).astype(np.float32)
    for mode in ('solid_angle', 'uniform'):
        wt = ops.sphere_eval_weights(h, mode, torch.device(DEV, torch.cuda.current_device()))
        pos = M.astype(np.int32)
        neg = (wt.cpu().numpy()[None, :, None] * (1 - pos)).astype(np.int32)
        scores, n_fix = ops.sphere_eval(dev(S), dev(G), wt, fixations=dev(M.astype(np.uint8)))
        got = ops.shuffled_auc(dev(S), dev(pos), dev(neg))
        auc = assert_sauc(got, S, pos, neg)                            # ... and both are the exact quotient
        assert np.isnan(auc).tolist() == [False, False, True] and n_fix.tolist() == M.sum(axis=(1, 2)).tolist()
        judd = scores[:, 0].contiguous()
        assert torch.equal(judd.view(torch.int64), got[0].view(torch.int64)), (mode, judd.tolist(), got[0].tolist())
        assert torch.equal(judd[:2], got[0][:2]) and bool(torch.isnan(judd[2])) and bool(torch.isnan(got[0][2]))


def rank_split(n, P):
    """K15d's launch rule, restated: the grid has ceil(P / 256) workgroups per frame, a frame's n positives fill
    `tiles` of them, and the pixel loop is split over chunks = min(grid / tiles, max(1, P / (kSplit n))) workgroups per tile
    -> (tiles, chunks, the workgroups that return at once).  kSplit is read from the source: tuning it must not move the
    test's frames off the branches unnoticed."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(ops.__file__), 'csrc', 'fixations.hip')).read()
    k_split = int(re.search(r'constexpr int kSplit = (\d+);', src).group(1))
    grid, tiles = -(-P // 256), -(-n // 256)
    chunks = min(grid // tiles, max(1, P // (k_split * n)))
    return tiles, chunks, grid - tiles * chunks


def split_inputs(hw, counts):
    """One frame per entry of `counts`, with exactly that many positive pixels (multiplicities 1 .. 3), quantised and
    continuous maps in turn, negatives 0 .. 4 on every pixel."""
    h, w = hw
    F, P = len(counts), h * w
    S = hashrng.uniform(1890 + h, (F, h, w), 0.0, 1.0, dtype=np.float64).astype(np.float32)
    S[::2] = fr.quantised(1891 + h, F, h, w, 8)[::2]
    pos = np.zeros((F, P), np.int32)
    for f, n in enumerate(counts):
        where = np.argsort(hashrng.uniform(1892 + h + f, (P,), 0.0, 1.0, dtype=np.float64))[:n]
        pos[f, where] = hashrng.integers(1895 + h + f, (n,), 1, 4)
    neg = hashrng.integers(1898 + h, (F, h, w), 0, 5).astype(np.int32)
    return S, pos.reshape(F, h, w), neg


def test_sauc_on_every_branch_of_the_split_rule():
    """33 x 66: P = 2178, 9 workgroups per frame, 3 pixel tiles.  n = 1 and 3: one tile of positives, the pixel loop split over
    the spare workgroups (more chunks than pixel tiles: the last ones add nothing); n = 8: the split held back by kSplit, the
    rest return; n = 30: one tile and no split; n = 300: two tiles, no split, spare workgroups return; n = P - 1: every workgroup
    owns a tile.  8 x 16: one workgroup, nothing to split."""
    hw, P = (33, 66), 33 * 66
    counts = [1, 3, 8, 30, 300, P - 1]
    splits = [rank_split(n, P) for n in counts]
    print('split rule at 33 x 66 (tiles, chunks, returning):', splits)
    assert all(t == 1 and c > 1 for t, c, _ in splits[:2])
    assert splits[4][0] == 2 and splits[4][1] == 1 and splits[4][2] > 0
    assert splits[5] == (9, 1, 0)
    assert any(t == 1 and c == 1 for t, c, _ in splits) and any(t == 1 and c > 1 and r > 0 for t, c, r in splits)
    S, pos, neg = split_inputs(hw, counts)
    assert (pos > 0).sum(axis=(1, 2)).tolist() == counts
    auc = assert_sauc(ops.shuffled_auc(dev(S), dev(pos), dev(neg)), S, pos, neg)
    assert not np.isnan(auc).any()
    assert rank_split(1, 8 * 16) == (1, 1, 0)
    S, pos, neg = split_inputs((8, 16), [1])
    auc = assert_sauc(ops.shuffled_auc(dev(S), dev(pos), dev(neg)), S, pos, neg)
    assert not np.isnan(auc).any()


# ----------------------------------------------------------------------------- end to end
def test_fixation_maps_end_to_end(tmp_path):
    F, fps, viewers = 3, 10.0, 12
    t = np.arange(0.0, 0.45, 0.05)
    tracks = []
    for v in range(viewers):
        lon = 1.0 + 0.3 * t + 0.05 * hashrng.normal(1820 + v, t.shape, dtype=np.float64)
        lat = 0.4 - 0.2 * t + 0.05 * hashrng.normal(1840 + v, t.shape, dtype=np.float64)
        tracks.append((t, lon, lat))
    lonlat, offsets = fixations.scanpaths_to_points(tracks, fps, F)
    assert np.diff(offsets).tolist() == [viewers] * F
    fm = fixations.FixationMaps(grid_hw=(33, 66), sigma_deg=5.0, device=DEV)
    counts, n = fm.counts(lonlat, offsets)
    want_counts, want_n = fr.bin_points(lonlat, offsets, 33, 66)
    assert torch.equal(counts.cpu().long(), torch.from_numpy(want_counts)) and n.tolist() == want_n.tolist()
    mask = fm.mask(lonlat, offsets)
    assert mask.dtype == torch.uint8 and torch.equal(mask.cpu(), torch.from_numpy((want_counts > 0).astype(np.uint8)))
    raw, gt, unit_mass = fm.density(lonlat, offsets, None), fm.density(lonlat, offsets), fm.density(lonlat, offsets, 'mass')
    want = fr.density64(lonlat, offsets, 33, 66, np.deg2rad(5.0))
    assert density_error(raw.cpu().numpy(), want) <= DENSITY_GATE[5.0]
    assert torch.equal(gt.amax(dim=(1, 2)).cpu(), torch.ones(F)) and torch.equal(gt, raw / raw.amax(dim=(1, 2))[:, None, None])
    a = torch.from_numpy(ops.shot_weights_host(33)[0]).double().to(DEV) / 1024.0
    mass = (unit_mass.double() * a[None, :, None]).sum(dim=(1, 2)).cpu().numpy()
    assert np.max(np.abs(mass - 1.0)) <= 1e-6
    paths = fixations.save_gt(str(tmp_path / 'gt'), 'clip', gt, first_frame_no=4)
    assert [p[-9:] for p in paths] == ['00004.npy', '00005.npy', '00006.npy'] and '/clip.mp4/' in paths[0]
    sal = (0.9 * gt + 0.02 * dev(hashrng.uniform(1860, (F, 33, 66), 0.0, 1.0))).cpu().numpy()
    for k in range(F):
        npy_io.save_saliency(str(tmp_path / 'pred'), 'clip', 4 + k, sal[k])
    ev = eval_sphere.SphereEval(grid_hw=(33, 66), device=DEV)
    r = eval_sphere.evaluate_video_dir(str(tmp_path / 'pred'), str(tmp_path / 'gt'), 'clip', ev)      # reads what save_gt wrote
    assert r.frames == [4, 5, 6] and bool((r.cc > 0.9).all())
    with_mask = ev.evaluate(sal, gt, fixations=mask)
    assert with_mask.n_fix.tolist() == (want_counts > 0).sum(axis=(1, 2)).tolist() and bool((with_mask.auc_judd > 0.9).all())
    auc, c_tot, a_neg = fm.shuffled_auc(sal, counts)
    neg = fr.other_frames(want_counts)
    want_auc = fr.sauc_video(sal.astype(np.float32), want_counts, neg)
    assert np.array_equal(auc.cpu().numpy(), want_auc[0]) and c_tot.tolist() == [viewers] * F and a_neg.tolist() == [2 * viewers] * F
    small = fm.shuffled_auc(sal[:, ::3, ::3], counts, negatives=counts.sum(dim=0))                     # resampled; one negative map
    assert tuple(small[0].shape) == (F,) and not torch.isnan(small[0]).any() and small[2].tolist() == [3 * viewers] * F
    work = fm._work                                                    # grown to three frames: kept from here on
    assert torch.equal(fm.density(lonlat, offsets), gt) and torch.equal(fm.shuffled_auc(sal, counts)[0], auc) and fm._work is work


# ----------------------------------------------------------------------------- refusals
def test_the_wrappers_refuse():
    lonlat, offsets = (dev(a) for a in fr.random_points(1870, [4, 3]))
    hw = (8, 16)
    for bad in (lonlat.float(), lonlat.reshape(-1), lonlat.t().contiguous().t(), lonlat[:, :1], lonlat.cpu()):
        with pytest.raises((ValueError, RuntimeError)):
            ops.fixation_counts(bad, offsets, hw)
        with pytest.raises((ValueError, RuntimeError)):
            ops.fixation_density(bad, offsets, hw, 0.1)
    for bad in (offsets.long(), offsets[:1], offsets.reshape(1, -1), offsets[::2]):
        with pytest.raises(ValueError):
            ops.fixation_counts(lonlat, bad, hw)
    for sigma in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            ops.fixation_density(lonlat, offsets, hw, sigma)
    with pytest.raises(ValueError):
        ops.fixation_counts(lonlat, offsets, (0, 16))
    with pytest.raises(ValueError):
        ops.fixation_density(lonlat, offsets, (1024, 2049), 0.1)
    S = torch.zeros((2,) + hw, device=DEV)
    pos = torch.ones((2,) + hw, dtype=torch.int32, device=DEV)
    for args in ((S.double(), pos, pos), (S, pos.long(), pos), (S, pos, pos.long()), (S[0], pos[0], pos[0]), (S, pos[:1], pos),
                 (S, pos, torch.cat([pos, pos])), (S.transpose(1, 2), pos.transpose(1, 2), pos.transpose(1, 2)), (S, pos.cpu(), pos)):
        with pytest.raises((ValueError, RuntimeError)):
            ops.shuffled_auc(*args)
    fm = fixations.FixationMaps(grid_hw=hw, device=DEV)
    with pytest.raises(ValueError):
        fm.density(lonlat, offsets, normalize='sum')
    with pytest.raises(ValueError):
        fm.shuffled_auc(S, pos, negatives='all_frames')
    with pytest.raises(ValueError):
        fm.shuffled_auc(S, pos.float())
    with pytest.raises(ValueError):
        fm.shuffled_auc(S, pos, negatives=pos)                          # a negative map is [h, w]
