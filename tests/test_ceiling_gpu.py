"""The point scores behind the human ceiling and the prior baselines on the GPU (K19, csrc/fixations.hip) against the numpy
restatement of their specification (tests/ceiling_restate.py, whose own claims tests/test_ceiling_cpu.py pins).

Tolerances.  Map mode compares float32 values, which float64 holds exactly: the AUC is one quotient of integers, bit-equal to the
restatement's quotient of Python integers and to ``ops.sphere_eval``'s AUC-Judd of a one-pixel mask; the NSS is a quotient of
sums of at most 28 800 float64 terms: K14's 1e-9, relative or absolute.  Leave-one-out mode scores maps whose terms are float32
expf values: a comparison that the density gate of the sigma cannot decide (ceiling_restate.point_band) may fall either way, so
the AUC is held between the restatement's quotient with those comparisons counted in and counted out - test_ceiling_cpu.py caps
how many there are - and the NSS to the float64 definition within NSS_GATE[sigma] (below), relative.  Batch, chunk, stream and
workspace independence: torch.equal."""
import functools
import math

import numpy as np
import pytest
import torch

from cp_360_weakly_supervised_saliency_amd import _lib, ops
from cp_360_weakly_supervised_saliency_amd.utils import fixations, hashrng
from tests import ceiling_restate as cr
from tests import fixations_restate as fr
from tests import sphere_eval_restate as rs

pytestmark = pytest.mark.gpu
DEV = 'cuda'
# The largest relative error of a point's leave-one-out NSS against the float64 definition over the cases of
# ceiling_restate.LOO_CASES, per sigma.  It is the density's error (test_fixations_gpu.DENSITY_MEASURED: the float32 rounding of
# the dot product times kappa) carried through two weighted sums and a quotient.  Measured (the float32-term restatement on the
# CPU = density32's operations; the kernel on an MI355X):
NSS_MEASURED = {5.0: (8.988e-6, 8.999e-6), 10.0: (2.984e-6, 2.987e-6), 20.0: (6.510e-7, 6.657e-7)}
# The gate is four times the larger of the two, as the density's: expf and the rounding of q may differ by a few ulp between the
# device and numpy.  A dropped or doubled viewer moves a point's NSS by about 1 / n of itself, 3e-3 at 300 viewers: four times the
# rounding cannot hide one.
NSS_GATE = {s: 4.0 * max(m) for s, m in NSS_MEASURED.items()}


def dev(a):
    return torch.from_numpy(np.array(a, order='C')).to(DEV)            # a copy: the shared inputs are read-only


def weights_dev(a_rows):
    return dev(np.asarray(a_rows, np.int32))


def loo(lonlat, offsets, hw, a_rows, sigma_deg, **kw):
    return ops.fixation_point_scores(dev(np.asarray(lonlat, np.float64).reshape(-1, 2)), dev(np.asarray(offsets, np.int32)), hw,
                                     weights_dev(a_rows), sigma_rad=np.deg2rad(sigma_deg), **kw)


def by_map(S, lonlat, offsets, hw, a_rows, **kw):
    return ops.fixation_point_scores(dev(np.asarray(lonlat, np.float64).reshape(-1, 2)), dev(np.asarray(offsets, np.int32)), hw,
                                     weights_dev(a_rows), maps=dev(S), **kw)


def same_bits(a, b):
    """torch.equal on the bits of two float64 tensors: NaN rows compare too (the library and torch write one NaN)."""
    return a.dtype == b.dtype == torch.float64 and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def nss_error(got, want):
    ok = ~np.isnan(want)
    assert np.array_equal(np.isnan(got), ~ok)
    return float(np.max(np.abs(got[ok] - want[ok]) / np.abs(want[ok]))) if ok.any() else 0.0


def assert_loo(got, s, s32, offsets, sigma_deg, what):
    """got f64 [N, 2] (device) against the restated scores s (float64 terms, with the band) and s32 (float32 terms)."""
    assert got.dtype == torch.float64 and tuple(got.shape) == (len(s['auc']), 2)
    got = got.cpu().numpy()
    n = np.diff(np.asarray(offsets))
    per = np.repeat(n, n)
    scored = ~np.isnan(s['auc'])
    assert np.array_equal(np.isnan(got[:, 0]), ~scored)
    alone = scored & (per == 1)
    assert np.all(got[alone, 0] == 0.5) and np.isnan(got[alone, 1]).all()      # a viewer alone: every pixel ties at 0
    m = scored & (per > 1)
    assert np.all(s['auc_lo'][m] <= got[m, 0]) and np.all(got[m, 0] <= s['auc_hi'][m])
    cpu, gpu = nss_error(s32['nss'], s['nss']), nss_error(got[:, 1], s['nss'])
    print('%s sigma %g: NSS float32 restatement %.3e, kernel %.3e relative (gate %.3e); AUC differs from float64 at %d of %d points'
          % (what, sigma_deg, cpu, gpu, NSS_GATE[sigma_deg], int(np.sum(got[m, 0] != s['auc'][m])), int(m.sum())))
    assert cpu <= NSS_GATE[sigma_deg] and gpu <= NSS_GATE[sigma_deg]


# ----------------------------------------------------------------------------- leave-one-out mode
@pytest.mark.parametrize('name', sorted(cr.LOO_CASES))
def test_leave_one_out_against_the_restatement(name):
    h, w, sigma_deg, _, per_frame = cr.LOO_CASES[name]
    lonlat, offsets, a_rows = cr.loo_case(name)
    got = loo(lonlat, offsets, (h, w), a_rows, sigma_deg)
    assert_loo(got, cr.loo_case_scores(name), cr.loo_case_scores(name, True), offsets, sigma_deg, name)
    assert int(torch.isnan(got[:, 0]).sum()) == 0 and len(got) == len(lonlat) >= sum(per_frame)


def test_dropped_points_get_nan_and_leave_their_neighbours_bits():
    h, w, sigma_deg = 33, 66, 5.0
    lonlat, offsets, a_rows = cr.loo_case('odd')
    clean = loo(lonlat, offsets, (h, w), a_rows, sigma_deg)
    dirty = np.insert(lonlat, [75, 100], [[np.nan, 0.1], [0.3, -np.inf]], axis=0)         # both in the second frame
    got = loo(dirty, [0, 70, 142, 212], (h, w), a_rows, sigma_deg)
    assert torch.isnan(got[75]).all() and torch.isnan(got[101]).all()
    keep = [k for k in range(212) if k not in (75, 101)]
    assert torch.equal(got[keep], clean)


def test_identical_points_and_points_that_share_a_pixel():
    h, w, sigma_deg = cr.LOO_CASES['twins'][:3]
    pts, offsets, a_rows = cr.loo_case('twins')                        # point 12 is point 0 again, point 13 lies in point 1's pixel
    pix = cr.point_pixels(pts, h, w)[1]
    assert np.array_equal(pts[12], pts[0]) and pix[13] == pix[1] and not np.array_equal(pts[13], pts[1])
    got = loo(pts, offsets, (h, w), a_rows, sigma_deg)
    assert torch.equal(got[0], got[12]) and not torch.equal(got[1], got[13])
    assert_loo(got, cr.loo_case_scores('twins'), cr.loo_case_scores('twins', True), offsets, sigma_deg, 'twins')


def test_scattered_points_stay_within_their_bounds():
    """Viewers far from every other one: their map underflows to 0 over most of the sphere and ties there, so the band is wide and
    the cap of test_ceiling_cpu.py does not hold - the bounds still do."""
    h, w, sigma_deg = 30, 60, 5.0
    lonlat, offsets = fr.random_points(1906, [20, 5])
    a_rows = rs.weights(h)
    got = loo(lonlat, offsets, (h, w), a_rows, sigma_deg).cpu().numpy()
    s = cr.loo_scores(lonlat, offsets, h, w, np.deg2rad(sigma_deg), a_rows, False, cr.DENSITY_REL[sigma_deg])
    assert np.all(s['auc_lo'] <= got[:, 0]) and np.all(got[:, 0] <= s['auc_hi'])
    assert np.all(got[:, 0] >= 0.0) and np.all(got[:, 0] <= 1.0) and np.isfinite(got[:, 1]).all()
    print('scattered: the band is %.3f wide on average' % float(np.mean(s['auc_hi'] - s['auc_lo'])))


# ----------------------------------------------------------------------------- map mode
@functools.lru_cache(maxsize=None)
def map_case():
    """(S f32 [3, 33, 66], the points of 'odd'): continuous values."""
    S = hashrng.uniform(1910, (3, 33, 66), 0.0, 1.0, dtype=np.float64).astype(np.float32)
    S.setflags(write=False)
    return S


def assert_maps(got, want, what):
    got = got.cpu().numpy()
    assert np.array_equal(got[:, 0], want[0], equal_nan=True), what    # one quotient of integers
    ok = ~np.isnan(want[1])
    assert np.array_equal(np.isnan(got[:, 1]), ~ok)
    err = np.abs(got[ok, 1] - want[1][ok]) / np.maximum(1.0, np.abs(want[1][ok]))
    print('%s: NSS apart %.2e at most' % (what, err.max() if err.size else 0.0))
    assert np.all(err <= 1e-9), what


@pytest.mark.parametrize('weights', ['solid_angle', 'uniform'])
def test_maps_against_the_restatement(weights):
    h, w = 33, 66
    lonlat, offsets, _ = cr.loo_case('odd')
    a_rows, S = rs.weights(h, weights), map_case()
    assert_maps(by_map(S, lonlat, offsets, (h, w), a_rows), cr.map_scores(S, lonlat, offsets, h, w, a_rows), 'a map per frame')
    assert_maps(by_map(S[1:2], lonlat, offsets, (h, w), a_rows), cr.map_scores(S[1:2], lonlat, offsets, h, w, a_rows), 'one map')
    Q = fr.quantised(1911, 3, h, w)                                    # 8 levels: ties everywhere
    assert_maps(by_map(Q, lonlat, offsets, (h, w), a_rows), cr.map_scores(Q, lonlat, offsets, h, w, a_rows), 'quantised')


@pytest.mark.parametrize('hw', [(5, 9), (33, 66), (120, 240)])
def test_a_one_point_frame_is_sphere_eval_with_that_pixel_fixated(hw):
    h, w = hw
    F = 3
    a_rows = rs.weights(h)
    lonlat, offsets = fr.random_points(1912, [1] * F)
    S = np.concatenate([hashrng.uniform(1913, (2, h, w), 0.0, 1.0, dtype=np.float64).astype(np.float32), fr.quantised(1914, 1, h, w)])
    got = by_map(S, lonlat, offsets, hw, a_rows)
    M = (fr.bin_points(lonlat, offsets, h, w)[0] > 0).astype(np.uint8)
    scores, n_fix = ops.sphere_eval(dev(S), dev(S), weights_dev(a_rows), dev(M))
    assert n_fix.tolist() == [1] * F
    assert torch.equal(got[:, 0], scores[:, 0]) and not torch.isnan(got).any()
    assert torch.all((got[:, 1] - scores[:, 1]).abs() <= 1e-9 * scores[:, 1].abs().clamp(min=1.0))
    assert_maps(got, cr.map_scores(S, lonlat, offsets, h, w, a_rows), 'one point a frame')


def test_a_flat_map_ties_every_pixel():
    h, w = 12, 24
    lonlat, offsets, a_rows = cr.loo_case('small')
    got = by_map(np.full((1, h, w), 0.25, np.float32), lonlat, offsets, (h, w), a_rows)
    assert torch.all(got[:, 0] == 0.5) and torch.isnan(got[:, 1]).all()


@pytest.mark.parametrize('f', [0, 2, 4])
def test_a_non_finite_map_spoils_its_frame_alone(f):
    h, w = 12, 24
    lonlat, offsets, a_rows = cr.loo_case('small')
    S = hashrng.uniform(1915, (5, h, w), 0.0, 1.0, dtype=np.float64).astype(np.float32)
    clean = by_map(S, lonlat, offsets, (h, w), a_rows)
    for bad in (np.nan, np.inf):
        Sb = S.copy()
        Sb[f, h - 1, w - 1] = bad
        got = by_map(Sb, lonlat, offsets, (h, w), a_rows)
        rows = torch.zeros(len(lonlat), dtype=torch.bool, device=DEV)
        rows[offsets[f]:offsets[f + 1]] = True
        assert torch.isnan(got[rows]).all() and torch.equal(got[~rows], clean[~rows])


# ----------------------------------------------------------------------------- plumbing
def test_a_frame_does_not_depend_on_the_batch_the_place_or_the_run():
    h, w, sigma_deg = 33, 66, 5.0
    lonlat, offsets, a_rows = cr.loo_case('odd')
    S = map_case()
    batch, again = loo(lonlat, offsets, (h, w), a_rows, sigma_deg), loo(lonlat, offsets, (h, w), a_rows, sigma_deg)
    assert torch.equal(batch, again)
    one = lonlat[70:140]                                               # the second frame alone, and fifth of seven
    moved = np.concatenate([lonlat[140:], lonlat[:70], lonlat[:3], one, lonlat[140:150]])
    offs = [0, 70, 140, 140, 143, 213, 223, 223]
    alone, fifth = loo(one, [0, 70], (h, w), a_rows, sigma_deg), loo(moved, offs, (h, w), a_rows, sigma_deg)
    assert torch.equal(alone, batch[70:140]) and torch.equal(fifth[143:213], batch[70:140]) and torch.equal(fifth[:70], batch[140:])
    maps = by_map(S, lonlat, offsets, (h, w), a_rows)
    Sm = np.stack([S[2], S[0], S[0], S[0], S[1], S[2], S[2]])
    assert torch.equal(by_map(S[1:2], one, [0, 70], (h, w), a_rows), maps[70:140])
    assert torch.equal(by_map(Sm, moved, offs, (h, w), a_rows)[143:213], maps[70:140])


def test_ceiling_in_two_chunks_is_one_call():
    h, w, F = 12, 24, 300
    lonlat, offsets, _ = fr.prior_video(1907, F, 6, h, w)
    lonlat[7] = np.nan                                                 # a dropped point; the third frame loses all but one
    keep = np.r_[0:13, 18:len(lonlat)]
    lonlat, offsets = np.ascontiguousarray(lonlat[keep]), np.r_[offsets[:3], offsets[3:] - 5].astype(np.int32)
    fm = fixations.FixationMaps(grid_hw=(h, w), sigma_deg=20.0)
    assert F > fixations.POINT_CHUNK
    r = fm.ceiling(lonlat, offsets)
    want = loo(lonlat, offsets, (h, w), rs.weights(h), 20.0)
    assert same_bits(r.auc, want[:, 0]) and same_bits(r.nss, want[:, 1]) and tuple(r.frame_auc.shape) == (F,)
    assert fm._work.numel() * 8 == _lib.lib().cp360_fix_point_work_bytes(fixations.POINT_CHUNK, h, w)
    host = want.cpu().numpy()
    for c, (frame, video) in enumerate(((r.frame_auc, r.video_auc), (r.frame_nss, r.video_nss))):
        fm_want, vm_want = cr.video_means(host[:, c], offsets)
        assert np.allclose(frame.cpu().numpy(), fm_want, rtol=1e-12, atol=0.0, equal_nan=True) and abs(float(video) - vm_want) <= 1e-12 * abs(vm_want)
    assert math.isnan(float(r.frame_nss[2])) and float(r.frame_auc[2]) == 0.5 and math.isnan(float(r.nss[7]))
    again = fm.ceiling(dev(lonlat), dev(offsets))                      # device points, the workspace reused
    assert same_bits(again.auc, r.auc) and same_bits(again.frame_nss, r.frame_nss) and same_bits(again.video_auc, r.video_auc)
    # the maps of a model, a chunk at a time, at another size: resampled as shuffled_auc resamples them
    sal = hashrng.uniform(1908, (F, 2 * h, 2 * w), 0.0, 1.0, dtype=np.float64).astype(np.float32)
    S = ops.sphere_eval_resample(dev(sal), (h, w))
    m = fm.score_points(sal, lonlat, offsets)
    want = ops.fixation_point_scores(dev(lonlat), dev(offsets), (h, w), weights_dev(rs.weights(h)), maps=S)
    assert same_bits(m.auc, want[:, 0]) and same_bits(m.nss, want[:, 1])
    one = fm.score_points(sal[5], lonlat, offsets, weights='uniform')
    want = ops.fixation_point_scores(dev(lonlat), dev(offsets), (h, w), weights_dev(rs.weights(h, 'uniform')), maps=S[5:6])
    assert same_bits(one.auc, want[:, 0]) and same_bits(one.nss, want[:, 1])


def test_another_stream_and_a_workspace_full_of_nan():
    h, w, sigma_deg = 33, 66, 5.0
    lonlat, offsets, a_rows = cr.loo_case('odd')
    S = map_case()
    want, want_m = loo(lonlat, offsets, (h, w), a_rows, sigma_deg), by_map(S, lonlat, offsets, (h, w), a_rows)
    device = torch.device(DEV, torch.cuda.current_device())
    work = torch.full_like(ops.fixation_point_work(3, h, w, device), float('nan'))
    assert torch.equal(loo(lonlat, offsets, (h, w), a_rows, sigma_deg, work=work), want)
    work.fill_(float('nan'))
    assert torch.equal(by_map(S, lonlat, offsets, (h, w), a_rows, work=work), want_m)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got, got_m = loo(lonlat, offsets, (h, w), a_rows, sigma_deg), by_map(S, lonlat, offsets, (h, w), a_rows)
    side.synchronize()
    assert torch.equal(got, want) and torch.equal(got_m, want_m)


def test_a_small_workspace_is_refused_and_no_points_are_fine():
    h, w = 12, 24
    lonlat, offsets, a_rows = cr.loo_case('small')
    L = _lib.lib()
    ll, off, a = dev(lonlat), dev(offsets), weights_dev(a_rows)
    need = L.cp360_fix_point_work_bytes(5, h, w)
    work = torch.empty(need // 8, dtype=torch.float64, device=DEV)
    scores = torch.full((len(lonlat), 2), 7.0, dtype=torch.float64, device=DEV)
    st = L.cp360_fix_point_scores(None, 0, _lib.ptr(ll), _lib.ptr(off), len(lonlat), 5, h, w, 0.3, _lib.ptr(a), _lib.ptr(scores),
                                  _lib.ptr(work), need - 8, _lib.stream())
    torch.cuda.synchronize()
    assert st == -1 and torch.all(scores == 7.0)                       # refused before any launch
    empty = torch.zeros((0, 2), dtype=torch.float64, device=DEV)
    zeros = torch.zeros(4, dtype=torch.int32, device=DEV)
    assert tuple(ops.fixation_point_scores(empty, zeros, (h, w), a, sigma_rad=0.3).shape) == (0, 2)
    assert tuple(ops.fixation_point_scores(empty, zeros, (h, w), a, maps=torch.zeros((1, h, w), device=DEV)).shape) == (0, 2)
    r = fixations.FixationMaps(grid_hw=(h, w)).ceiling(np.zeros((0, 2)), np.zeros(4, np.int32))
    assert tuple(r.auc.shape) == (0,) and torch.isnan(r.frame_auc).all() and math.isnan(float(r.video_nss))
    # offsets are clamped as K15 clamps them; a point that no frame owns has no score
    got = ops.fixation_point_scores(ll, dev(np.array([-5, 12, 24, 99], np.int32)), (h, w), a, sigma_rad=np.deg2rad(20.0))
    want = loo(lonlat[:24], [0, 12, 24], (h, w), a_rows, 20.0)
    assert torch.equal(got[:24], want) and not torch.isnan(got[24:]).any()
    got = ops.fixation_point_scores(ll, dev(np.array([12, 24], np.int32)), (h, w), a, sigma_rad=np.deg2rad(20.0))
    assert torch.isnan(got[:12]).all() and torch.isnan(got[24:]).all() and torch.equal(got[12:24], want[12:24])


def test_the_wrappers_refuse_what_the_library_would():
    h, w = 12, 24
    lonlat, offsets, a_rows = cr.loo_case('small')
    ll, off, a = dev(lonlat), dev(offsets), weights_dev(a_rows)
    S = torch.zeros((5, h, w), device=DEV)
    for sg in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='sigma_rad'):
            ops.fixation_point_scores(ll, off, (h, w), a, sigma_rad=sg)
    for bad in (S[:2], S[:, :-1], S.double(), S.transpose(1, 2), S[0]):
        with pytest.raises(ValueError):
            ops.fixation_point_scores(ll, off, (h, w), a, maps=bad)
    for bad in (a[:-1], a.long(), a.cpu()):
        with pytest.raises((ValueError, RuntimeError)):
            ops.fixation_point_scores(ll, off, (h, w), bad, sigma_rad=0.3)
    with pytest.raises(ValueError, match='lonlat'):
        ops.fixation_point_scores(ll.float(), off, (h, w), a, sigma_rad=0.3)
    with pytest.raises(ValueError, match='unsupported geometry'):
        ops.fixation_point_scores(ll, off, (1024, 2049), torch.zeros(1024, dtype=torch.int32, device=DEV), sigma_rad=0.3)
    fm = fixations.FixationMaps(grid_hw=(h, w))
    one = lonlat[:12].copy()                                           # the shared inputs are read-only
    with pytest.raises(ValueError, match='F >= 2'):
        fm.prior(one, np.array([0, 12], np.int32))
    assert tuple(fm.prior(one, np.array([0, 12], np.int32), exclude_own=False).shape) == (h, w)


# ----------------------------------------------------------------------------- end to end
def test_baselines_of_a_video_with_an_equator_prior():
    """prior_video(1900, 24, 12, 30, 60) at 5 degrees: the ceiling lies above the prior, the frames' own densities lie at or above
    the ceiling (they have seen the viewer who is scored), so their normalised scores are above 1.  In float64 on the CPU
    (test_ceiling_cpu.py): ceiling 0.9971 / 9.13, own densities 0.9982 / 10.79, the other frames' prior 0.9067 / 1.12."""
    F, h, w = 24, 30, 60
    lonlat, offsets, equator = fr.prior_video(1900, F, 12, h, w)
    fm = fixations.FixationMaps(grid_hw=(h, w), sigma_deg=5.0)
    D = fm.density(lonlat, offsets, None)
    rows = fm.baselines(lonlat, offsets, sal=D)
    assert sorted(rows) == ['ceiling', 'model', 'normalised', 'prior'] and sorted(fm.baselines(lonlat, offsets)) == ['ceiling', 'prior']
    rows = {k: tuple(float(x) for x in v) for k, v in rows.items()}
    print(', '.join('%s AUC %.4f NSS %.2f' % ((k,) + v) for k, v in rows.items()))
    eq = fm.score_points(equator, lonlat, offsets)
    for c in range(2):
        assert rows['ceiling'][c] > rows['prior'][c] and rows['ceiling'][c] > float((eq.video_auc, eq.video_nss)[c])
        assert rows['model'][c] >= rows['ceiling'][c] and rows['normalised'][c] > 1.0
        assert rows['normalised'][c] == (rows['model'][c] - rows['prior'][c]) / (rows['ceiling'][c] - rows['prior'][c])
    mean = fm.prior(lonlat, offsets, exclude_own=False)
    assert mean.dtype == torch.float32 and tuple(mean.shape) == (h, w)
    assert torch.allclose(mean, D.to(torch.float64).mean(dim=0).to(torch.float32), rtol=1e-6, atol=1e-30)     # one float32 rounding apart at most
    others = fm.prior(lonlat, offsets)
    want = ((D.sum(dim=0, dtype=torch.float64)[None] - D) / (F - 1)).to(torch.float32)
    assert others.dtype == torch.float32 and tuple(others.shape) == (F, h, w) and torch.equal(others, want)
    p = fm.score_points(others, lonlat, offsets)
    assert float(p.video_auc) == rows['prior'][0] and float(p.video_nss) == rows['prior'][1]
