"""Sphere-weighted saliency metrics (K14) without a GPU: the claims of the restatement (tests/sphere_eval_restate.py) that
tests/test_sphere_eval_gpu.py holds the kernels to, and the library's exports, status codes and weight table."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from cp_360_weakly_supervised_saliency_amd import _lib, ops
from cp_360_weakly_supervised_saliency_amd.utils import eval_sphere, hashrng
from tests import shots_restate
from tests import sphere_eval_restate as rs

K14 = ('cp360_seval_work_bytes', 'cp360_seval_resample', 'cp360_seval_scores')
NULL, BAD_SHAPE, ALIGN, UNSUPPORTED = -5, -1, -6, -8


def noise(seed, h, w):
    return hashrng.uniform(seed, (h, w), 0.0, 1.0, dtype=np.float64).astype(np.float32)


# ----------------------------------------------------------------------------- the restatement's own claims
@pytest.mark.parametrize('hw', [(8, 16), (33, 66)])
def test_uniform_cc_is_numpy_corrcoef(hw):
    S, G = noise(1401, *hw), noise(1402, *hw)
    G = (0.5 * S + 0.5 * G).astype(np.float32)
    sc, _ = rs.frame_scores(S, G, rs.weights(hw[0], 'uniform'))
    want = np.corrcoef(S.astype(np.float64).reshape(-1), G.astype(np.float64).reshape(-1))[0, 1]
    assert abs(sc['cc'] - want) <= 1e-12


@pytest.mark.parametrize('mode', ['solid_angle', 'uniform'])
def test_a_yaw_rotation_changes_nothing(mode):
    """Rolling S, G and M by whole columns moves no pixel to another row: the ROC points are the same integers (AUC bit-identical),
    the float64 sums differ by their order only."""
    h, w = 33, 66
    sal, gt = rs.video(1410, 1, h, w, h, w)
    a = rs.weights(h, mode)
    M = rs.derive_mask(gt[0], a)
    base, n = rs.frame_scores(sal[0], gt[0], a, M)
    assert 0 < n < h * w
    for k in (1, 7, 33, 65):
        r, nr = rs.frame_scores(np.roll(sal[0], k, 1), np.roll(gt[0], k, 1), a, np.roll(M, k, 1))
        assert nr == n and r['auc'] == base['auc']
        for name in ('nss', 'cc', 'sim', 'kl'):
            assert abs(r[name] - base[name]) <= 1e-12, (name, k)
        d, nd = rs.frame_scores(np.roll(sal[0], k, 1), np.roll(gt[0], k, 1), a)        # the derived mask rolls with G
        assert nd == n and d['auc'] == base['auc']


def blob_cc(h, w, lat, mode):
    S = rs.blob(h, w, rs.at_latitude(lat, 10.0), 15.0).astype(np.float32)
    G = rs.blob(h, w, rs.at_latitude(lat, -10.0), 12.0).astype(np.float32)
    return rs.frame_scores(S, G, rs.weights(h, mode))[0]['cc']


def test_solid_angle_cc_does_not_depend_on_the_resolution():
    """Two analytic blobs 20 degrees of longitude apart, sampled at 60 x 120 and at 120 x 240.  With solid-angle weights the CC
    is a midpoint quadrature of the same integrals over the sphere: it moves by at most 5e-4 between the two grids (measured:
    5.1e-6 at latitude 0, 4.9e-7 at 40, 6.8e-5 at 75 degrees, where a blob of 12 degrees spans the fewest columns' worth of solid
    angle).  Uniform weights answer another question - at 75 degrees, where a row covers a quarter of the equator's solid angle,
    they move the CC by 1.65e-2 (measured; asserted: more than 5e-3, ten times the margin, and more than the resolution does)."""
    for lat in (0.0, 40.0, 75.0):
        lo, hi = blob_cc(60, 120, lat, 'solid_angle'), blob_cc(120, 240, lat, 'solid_angle')
        print('latitude %g: solid-angle CC %.6f at 60 x 120, %.6f at 120 x 240, apart %.2e' % (lat, lo, hi, abs(lo - hi)))
        assert abs(lo - hi) <= 5e-4
    sa, un = blob_cc(120, 240, 75.0, 'solid_angle'), blob_cc(120, 240, 75.0, 'uniform')
    print('latitude 75: uniform CC %.6f against %.6f, apart %.2e' % (un, sa, abs(un - sa)))
    assert abs(un - sa) > 5e-3 and abs(un - sa) > abs(blob_cc(60, 120, 75.0, 'solid_angle') - sa)


def test_auc_prefers_the_map_itself():
    h, w = 33, 66
    _, gt = rs.video(1420, 1, h, w, h, w)
    a = rs.weights(h)
    own = rs.frame_scores(gt[0], gt[0], a)[0]
    turned = rs.frame_scores(np.roll(gt[0], w // 2, 1), gt[0], a)[0]
    assert own['auc'] > turned['auc'] and own['auc'] > 0.95
    assert abs(own['cc'] - 1.0) <= 1e-12 and abs(own['sim'] - 1.0) <= 1e-12 and abs(own['kl']) <= 1e-12
    assert own['nss'] > turned['nss']


@pytest.mark.parametrize('hw', [(8, 16), (12, 20)])
def test_roc_points_against_all_pairs(hw):
    """The sorted-array form of the ROC points against their definition, with and without ties; the trapezoid sum in float64
    against the one quotient of integers."""
    a = rs.weights(hw[0])
    M = noise(1430, *hw) > 0.8
    for S in (noise(1431, *hw), (np.floor(noise(1431, *hw) * 8.0) / 8.0).astype(np.float32)):
        A, c, a_neg = rs.roc_points(S, M, a)
        Ab, cb, a_neg_b = rs.roc_points_brute(S, M, a)
        assert np.array_equal(A, Ab) and np.array_equal(c, cb) and a_neg == a_neg_b
        assert np.all(np.diff(A) >= 0) and np.all(np.diff(c) >= 0) and c[-1] == M.sum()
        assert abs(rs.auc_trapezoid(A, c, a_neg, int(M.sum())) - rs.auc_exact(A, c, a_neg, int(M.sum()))) <= 1e-12


def test_quantised_maps_tie_inside_and_across_the_mask():
    h, w = 33, 66
    a = rs.weights(h)
    S = (np.floor(noise(1440, h, w) * 8.0) / 8.0).astype(np.float32)                 # 8 levels
    M = noise(1441, h, w) > 0.9
    A, c, a_neg = rs.roc_points(S, M, a)
    assert np.unique(S).size == 8 and np.unique(np.stack([A, c]), axis=1).shape[1] == 8            # tied fixations share a point
    for lvl in np.unique(S):
        assert (S[M] == lvl).sum() > 1 and (S[~M] == lvl).sum() > 1                                # ties straddle the mask
    sc, n = rs.frame_scores(S, noise(1442, h, w), a, M)
    assert n == M.sum() and 0.3 < sc['auc'] < 0.7
    # every level's point: the count and the weight of everything at or above the level
    aw = np.repeat(a[:, None], w, 1)
    for Ai, ci, lvl in zip(A, c, S[M][np.lexsort((np.flatnonzero(M.reshape(-1)), -S[M].astype(np.float64)))]):
        assert ci == (S[M] >= lvl).sum() and Ai == aw[(~M) & (S >= lvl)].sum()


@pytest.mark.parametrize('mode', ['solid_angle', 'uniform'])
def test_auc_judd_is_the_shuffled_auc_of_the_mask_and_the_unfixated_weights(mode):
    """K14's AUC is K15's shuffled AUC with pos = M and neg = a (1 - M): the quotients are bit-equal, on
    continuous maps and on quantised ones whose ties straddle the mask."""
    from tests import fixations_restate as fr
    for h, w in ((8, 16), (33, 66)):
        a = rs.weights(h, mode)
        M = noise(1470 + h, h, w) > 0.85
        neg = np.repeat(a[:, None], w, 1) * ~M
        for S in (noise(1471 + h, h, w), (np.floor(noise(1471 + h, h, w) * 8.0) / 8.0).astype(np.float32)):
            A, c, a_neg = rs.roc_points(S, M, a)
            want = fr.sauc_exact(S, M.astype(np.int64), neg)
            assert rs.auc_exact(A, c, a_neg, int(M.sum())) == want and 0.0 < want < 1.0
            assert rs.frame_scores(S, noise(1472, h, w), a, M, exact_auc=True)[0]['auc'] == want


def test_degenerate_frames():
    h, w = 8, 16
    a = rs.weights(h)
    S, G = noise(1450, h, w), noise(1451, h, w)
    nan = math.isnan
    none, every = np.zeros((h, w), bool), np.ones((h, w), bool)
    for M, n in ((none, 0), (every, h * w)):
        sc, got = rs.frame_scores(S, G, a, M)
        assert got == n and nan(sc['auc']) and nan(sc['nss'])
        assert all(math.isfinite(sc[k]) for k in ('cc', 'sim', 'kl'))
    flat = np.full((h, w), 0.5, np.float32)
    M = G > 0.8
    sc, _ = rs.frame_scores(flat, G, a, M)                             # no variance and no mass in S
    assert nan(sc['cc']) and nan(sc['nss']) and nan(sc['sim']) and nan(sc['kl'])
    assert sc['auc'] == 0.5                                            # every fixation ties with everything: one point at (1, 1)
    sc, n = rs.frame_scores(S, flat, a)                                # ... in G: no pixel exceeds mean + 2 std either
    assert n == 0 and all(nan(sc[k]) for k in rs.NAMES)
    for bad in (np.nan, np.inf, -np.inf):
        for which in (0, 1):
            maps = [S.copy(), G.copy()]
            maps[which][3, 5] = bad
            sc, _ = rs.frame_scores(maps[0], maps[1], a, M)
            assert all(nan(sc[k]) for k in rs.NAMES)
    allsc, counts = rs.scores(np.stack([S, flat, S]), np.stack([G, G, G]), a, np.stack([M, M, M]))
    one, _ = rs.scores(S[None], G[None], a, M[None])
    assert np.array_equal(allsc[0], one[0]) and np.array_equal(allsc[2], one[0]) and counts.tolist() == [M.sum()] * 3


def test_resample_restatement():
    src = noise(1460, 7, 14)[None]
    assert np.array_equal(rs.resample(src, 7, 14), src)
    up = rs.resample(src, 33, 66)
    assert up.dtype == np.float32 and up.shape == (1, 33, 66)
    assert src.min() <= up.min() and up.max() <= src.max()            # a convex combination
    # doubling: the grid's pixels lie a quarter of a source pixel off the source's centres; columns wrap, rows clamp
    up2 = rs.resample(src, 14, 28)[0].astype(np.float64)
    s = src[0].astype(np.float64)
    assert abs(up2[0, 0] - (0.75 * s[0, 0] + 0.25 * s[0, -1])) <= 1e-6
    assert abs(up2[5, 5] - (0.75 * (0.75 * s[2, 2] + 0.25 * s[2, 3]) + 0.25 * (0.75 * s[3, 2] + 0.25 * s[3, 3]))) <= 1e-6
    # a yaw by whole source columns commutes with the resampling
    assert np.array_equal(rs.resample(np.roll(src, 3, 2), 14, 28), np.roll(rs.resample(src, 14, 28), 6, 2))


# ----------------------------------------------------------------------------- library
def test_library_exports_the_symbols():
    L = _lib.lib()
    for name in K14:
        assert name in _lib.PUBLIC_SYMBOLS and hasattr(L, name)
    assert L.cp360_version() == 306


@pytest.mark.parametrize('h', [1, 8, 33, 120, 480])
def test_weight_table_is_k13s(h):
    a = ops.shot_weights_host(h)[0]
    assert np.array_equal(a, rs.weights(h)) and np.array_equal(a, shots_restate.weights(h)[0])
    assert np.array_equal(rs.weights(h, 'uniform'), np.full(h, 1024))
    dev = torch.device('cpu')
    assert np.array_equal(ops.sphere_eval_weights(h, 'solid_angle', dev).numpy(), a)
    assert ops.sphere_eval_weights(h, 'uniform', dev).dtype == torch.int32
    assert np.array_equal(ops.sphere_eval_weights(h, 'uniform', dev).numpy(), np.full(h, 1024))


def test_status_codes_without_gpu():
    """Argument validation happens before any launch: the dummy pointers are never used."""
    L = _lib.lib()
    one, big = C.c_void_p(16), 1 << 40
    scores = lambda S, G, fx, wt, F, h, w, sc, nf, wk, nb: L.cp360_seval_scores(S, G, fx, wt, F, h, w, sc, nf, wk, nb, None)
    ok = [one, one, None, one, 2, 8, 16, one, one, one, big]
    for k in (0, 1, 3, 7, 8, 9):
        args = list(ok)
        args[k] = None
        assert scores(*args) == NULL
    for F, h, w in ((0, 8, 16), (2, 0, 16), (2, 8, 0), (-1, 8, 16), (2, -8, 16), (2, 8, -16)):
        assert scores(one, one, None, one, F, h, w, one, one, one, big) == BAD_SHAPE
        assert L.cp360_seval_work_bytes(F, h, w) == 0
        assert L.cp360_seval_resample(one, F, h, w, one, 8, 16, None) == BAD_SHAPE
        assert L.cp360_seval_resample(one, 2 if F < 1 else F, 8, 16, one, h if F >= 1 else 0, w, None) == BAD_SHAPE
    assert scores(one, one, None, one, 65536, 8, 16, one, one, one, big) == UNSUPPORTED                 # grid y
    assert scores(one, one, None, one, 1, 1024, 2049, one, one, one, big) == UNSUPPORTED                # 1024 P >= 2^31
    assert L.cp360_seval_work_bytes(65536, 8, 16) == 0 and L.cp360_seval_work_bytes(1, 1024, 2049) == 0
    assert L.cp360_seval_work_bytes(1, 1024, 2048) > 0
    need = L.cp360_seval_work_bytes(2, 8, 16)
    assert need % 16 == 0 and need >= 2 * 8 * 16 * 20
    assert scores(one, one, None, one, 2, 8, 16, one, one, one, need - 1) == BAD_SHAPE                  # workspace too small
    assert scores(one, one, None, one, 2, 8, 16, one, one, C.c_void_p(8), big) == ALIGN
    assert scores(one, one, None, one, 2, 8, 16, C.c_void_p(4), one, one, big) == ALIGN
    assert L.cp360_seval_resample(None, 2, 4, 8, one, 8, 16, None) == NULL
    assert L.cp360_seval_resample(one, 2, 4, 8, None, 8, 16, None) == NULL
    assert L.cp360_seval_resample(one, 65536, 4, 8, one, 8, 16, None) == UNSUPPORTED
    assert L.cp360_seval_resample(one, 2, 4, 8, one, 1024, 2049, None) == UNSUPPORTED
    assert L.cp360_seval_resample(one, 2, 70000, 8, one, 8, 16, None) == UNSUPPORTED
    assert L.cp360_seval_resample(C.c_void_p(2), 2, 4, 8, one, 8, 16, None) == ALIGN


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    S = torch.zeros(2, 8, 16)
    wt = ops.sphere_eval_weights(8, 'solid_angle', 'cpu')
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.sphere_eval(S, S, wt)
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.sphere_eval_resample(S, (8, 16))
    with pytest.raises(ValueError):
        ops.sphere_eval_weights(8, 'cosine', 'cpu')
    with pytest.raises(ValueError):
        eval_sphere.SphereEval(weights='cosine')
    with pytest.raises(ValueError):
        eval_sphere.SphereEval(grid_hw=(0, 16))
    with pytest.raises(ValueError):
        eval_sphere.SphereEval(grid_hw=(1024, 2049))


def test_dataset_means_weigh_by_frames():
    per_video = [dict.fromkeys(eval_sphere.METRICS, 1.0), dict.fromkeys(eval_sphere.METRICS, 4.0)]
    per_video[1]['kl'] = -2.0
    got = eval_sphere.dataset_means(per_video, [30, 10])
    assert got['cc'] == pytest.approx(1.0 * 0.75 + 4.0 * 0.25, abs=1e-15) and got['kl'] == pytest.approx(0.75 - 0.5, abs=1e-15)
    assert set(got) == set(eval_sphere.METRICS)
    with pytest.raises(ValueError):
        eval_sphere.dataset_means(per_video, [30])
    with pytest.raises(ValueError):
        eval_sphere.dataset_means(per_video, [30, 0])
