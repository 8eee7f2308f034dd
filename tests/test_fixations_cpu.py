"""Fixation maps and shuffled AUC (K15) without a GPU: the claims of the restatement (tests/fixations_restate.py) that
tests/test_fixations_gpu.py holds the kernels to, the scan-path interpolation, and the library's exports and status codes."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from cp_360_weakly_supervised_saliency_amd import _lib, ops
from cp_360_weakly_supervised_saliency_amd.utils import fixations, hashrng
from tests import fixations_restate as fr
from tests import sphere_eval_restate as rs

K15 = ('cp360_fix_work_bytes', 'cp360_fix_counts', 'cp360_fix_density', 'cp360_fix_sauc')
NULL, BAD_SHAPE, ALIGN, UNSUPPORTED = -5, -1, -6, -8
PI = math.pi


# ----------------------------------------------------------------------------- binning
@pytest.mark.parametrize('hw', [(8, 16), (33, 66), (120, 240)])
def test_binning_edges(hw):
    h, w = hw
    lonlat, offsets, want = fr.edge_points(h, w)
    counts, n = fr.bin_points(lonlat, offsets, h, w)
    kept = [p for p in want if p is not None]
    assert int(n[0]) == len(kept) == int(counts.sum()) and len(kept) == len(want) - 5
    for k, p in enumerate(want):
        one, n1 = fr.bin_points(lonlat[k:k + 1], [0, 1], h, w)
        if p is None:
            assert int(one.sum()) == 0 and int(n1[0]) == 0, k
        else:
            assert int(one[0, p[1], p[0]]) == 1 and int(n1[0]) == 1, (k, p, np.argwhere(one[0]))


@pytest.mark.parametrize('hw', [(8, 16), (33, 66)])
def test_pixel_centres_land_in_their_pixel(hw):
    h, w = hw
    theta = ((2.0 * np.arange(w) + 1.0) / w - 1.0) * PI
    phi = (1.0 - (2.0 * np.arange(h) + 1.0) / h) * (PI / 2.0)
    lonlat = np.stack([np.tile(theta, h), np.repeat(phi, w)], -1)
    counts, n = fr.bin_points(lonlat, [0, h * w], h, w)
    assert np.array_equal(counts[0], np.ones((h, w), np.int64)) and int(n[0]) == h * w
    twice, _ = fr.bin_points(np.concatenate([lonlat, lonlat + [2.0 * PI, 0.0]]), [0, 2 * h * w], h, w)     # a turn further: the same pixels
    assert np.array_equal(twice[0], np.full((h, w), 2, np.int64))


# ----------------------------------------------------------------------------- density
def test_one_point_peaks_at_its_pixel():
    h, w = 33, 66
    for x, y in ((0, 0), (65, 32), (17, 5), (40, 30)):
        lon = ((2.0 * x + 1.0) / w - 1.0) * PI
        lat = (1.0 - (2.0 * y + 1.0) / h) * (PI / 2.0)
        for dens in (fr.density64, fr.density32):
            G = dens(np.array([[lon, lat]]), [0, 1], h, w, np.deg2rad(5.0))[0]
            assert np.unravel_index(np.argmax(G), G.shape) == (y, x) and abs(float(G[y, x]) - 1.0) <= 1e-6


def test_mass_on_the_sphere_and_why_a_flat_blur_is_wrong():
    """One point at latitude 0, 40 and 75 degrees on 120 x 240, sigma 10 degrees.  The solid-angle-weighted sum of the density
    times the pixel's solid angle is a midpoint quadrature of the kernel's integral over the sphere, 2 pi (1 - exp(-2 kappa)) /
    kappa: the grid's discretisation is all that separates them.  Measured with the float64 restatement, relative: 4.4e-16 at 0,
    7.4e-9 at 40 and 3.06e-4 at 75 degrees (the kernel's tail reaches the pole there, where the rows are coarse).  The gate is
    twice the largest of the three, 6.1e-4, computed here and not written down; the float32 density must meet it too (measured:
    1.5e-7, 1.9e-7, 3.06e-4).  A flat Gaussian of the same sigma in pixels, which is what blurring the equirectangular image
    gives, misses the same mass at 75 degrees by 0.740 (relative; 0.015 at the equator): a thousand times the gate."""
    h, w, sigma = 120, 240, np.deg2rad(10.0)
    want = fr.analytic_mass(sigma)
    gaps, gaps32 = [], []
    for lat_deg in (0.0, 40.0, 75.0):
        p = np.array([[np.deg2rad(20.0), np.deg2rad(lat_deg)]])
        gaps.append(abs(fr.sphere_mass(fr.density64(p, [0, 1], h, w, sigma)[0]) / want - 1.0))
        gaps32.append(abs(fr.sphere_mass(fr.density32(p, [0, 1], h, w, sigma)[0]) / want - 1.0))
    gate = 2.0 * max(gaps)
    print('mass gaps, float64: %.3e %.3e %.3e; float32: %.3e %.3e %.3e; gate %.3e' % (*gaps, *gaps32, gate))
    assert max(gaps32) <= gate
    flat = fr.flat_gaussian(np.deg2rad(20.0), np.deg2rad(75.0), h, w, sigma)
    miss = abs(fr.sphere_mass(flat) / want - 1.0)
    print('flat Gaussian at 75 degrees misses the mass by %.3e' % miss)
    assert miss > gate
    flat0 = abs(fr.sphere_mass(fr.flat_gaussian(np.deg2rad(20.0), 0.0, h, w, sigma)) / want - 1.0)
    print('flat Gaussian at the equator: %.3e' % flat0)
    assert flat0 < miss                                                # at the equator the flat blur is nearly right


def test_density_skips_non_finite_points_and_adds_frames_up():
    h, w, sigma = 8, 16, np.deg2rad(20.0)
    lonlat, offsets = fr.random_points(1601, [5, 0, 3])
    dirty = np.insert(lonlat, 2, [[np.nan, 0.0], [0.3, np.inf]], axis=0)
    for dens in (fr.density64, fr.density32):
        a = dens(lonlat, offsets, h, w, sigma)
        b = dens(dirty, offsets + np.array([0, 2, 2, 2], np.int32), h, w, sigma)
        assert np.array_equal(a, b) and not a[1].any() and a[0].min() > 0.0


# ----------------------------------------------------------------------------- shuffled AUC
def sauc_case(seed, h, w, levels=None, n_pos=12, max_pos=4):
    S = fr.quantised(seed, 1, h, w, levels)[0] if levels else hashrng.uniform(seed, (h, w), 0.0, 1.0, dtype=np.float64).astype(np.float32)
    pos = np.zeros(h * w, np.int64)
    idx = hashrng.integers(seed + 1, (n_pos,), 0, h * w)
    np.add.at(pos, idx, hashrng.integers(seed + 2, (n_pos,), 1, max_pos + 1))
    neg = hashrng.integers(seed + 3, (h, w), 0, 4) * (hashrng.integers(seed + 4, (h, w), 0, 3) == 0)
    return S, pos.reshape(h, w), neg


@pytest.mark.parametrize('levels', [None, 8, 2])
@pytest.mark.parametrize('hw', [(8, 16), (13, 31)])
def test_sauc_points_against_all_pairs(hw, levels):
    for seed in (1610, 1620, 1630):
        S, pos, neg = sauc_case(seed + hw[0], *hw, levels=levels)
        got, want = fr.sauc_points(S, pos, neg), fr.sauc_brute(S, pos, neg)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2:] == want[2:]
        assert np.all(np.diff(got[1]) > 0) and np.all(np.diff(got[0]) >= 0) and got[1][-1] == got[3]
        if levels:                                                     # ties: fewer points than positive pixels, and negatives tied with them
            assert len(got[0]) <= levels and len(got[0]) < int((pos > 0).sum())
            assert np.any((pos == 0) & (neg > 0) & np.isin(S, S[pos > 0]))


@pytest.mark.parametrize('levels', [None, 8])
def test_sauc_exact_is_the_trapezoid_sum(levels):
    for seed in (1640, 1650, 1660):
        S, pos, neg = sauc_case(seed, 33, 66, levels=levels, n_pos=60)
        A, Cc, a_neg, c_tot = fr.sauc_points(S, pos, neg)
        exact, trap = fr.sauc_exact(S, pos, neg), fr.sauc_trapezoid(A, Cc, a_neg, c_tot)
        print('exact %.17g trapezoid %.17g apart %.2e' % (exact, trap, abs(exact - trap)))
        assert 0.0 <= exact <= 1.0 and abs(exact - trap) <= 2e-16


def test_sauc_exact_agrees_with_the_float64_trapezoid_to_2e16():
    """A handful of ROC points: the float64 sum carries a rounding or two."""
    S, pos, neg = sauc_case(1670, 8, 16, levels=4, n_pos=6)
    A, Cc, a_neg, c_tot = fr.sauc_points(S, pos, neg)
    assert abs(fr.sauc_exact(S, pos, neg) - fr.sauc_trapezoid(A, Cc, a_neg, c_tot)) <= 2e-16


def by_parts_frames():
    """(name, S, pos, neg): quantised (8 levels) and unquantised maps at 8 x 16 and 33 x 66 with multiplicities up to 1023 and
    negatives up to 2^20 on every pixel class (positive or not, tied or not), a frame with a single positive, and a frame whose
    lowest positive value ties with negatives."""
    out = []
    for h, w in ((8, 16), (33, 66)):
        for levels in (8, None):
            seed = 1900 + 10 * h + (levels or 0)
            S, pos, _ = sauc_case(seed, h, w, levels=levels, n_pos=max(6, h * w // 20))
            pos = pos * hashrng.integers(seed + 5, (h, w), 1, 342)     # 3 * 341 = 1023; sauc_case gives 1 .. 4 and sums of them
            pos.reshape(-1)[np.flatnonzero(pos.reshape(-1))[:2]] = [1023, 2000]            # at the clamp and above it
            neg = hashrng.integers(seed + 6, (h, w), 0, (1 << 20) + 1) * (hashrng.integers(seed + 7, (h, w), 0, 3) > 0)
            neg.reshape(-1)[:2] = [1 << 20, 1 << 22]
            out.append(('%dx%d levels %s' % (h, w, levels), S, pos, neg))
            one = np.zeros_like(pos)
            one[h // 2, w // 3] = 7
            out.append(('%dx%d levels %s, a single positive' % (h, w, levels), S, one, neg))
        S, pos, neg = (a.copy() for a in out[-4][1:])                  # the quantised frame of this size
        low = np.flatnonzero(S.reshape(-1) == S.min())
        pos.reshape(-1)[low[0]] = 5
        neg.reshape(-1)[low[1:4]] = [3, 1 << 20, 0]
        assert S.reshape(-1)[np.flatnonzero(pos.reshape(-1))].min() == S.min() and np.any((pos == 0) & (neg > 0) & (S == S.min()))
        out.append(('%dx%d, the lowest positive ties with negatives' % (h, w), S, pos, neg))
    return out


def test_sauc_summed_by_parts_is_the_same_integer():
    """K15d adds up N = 2 A_neg C_tot - sum_k A_k (mult_k + mult_k+1); sauc_exact, the specification, divides the sum of
    (A_k - A_k-1)(C_k + C_k-1) over the points of sauc_points.  The two are the same Python integer."""
    frames = by_parts_frames()
    assert len(frames) == 10
    for name, S, pos, neg in frames:
        A, Cc, a_neg, c_tot = fr.sauc_points(S, pos, neg)
        want = fr.sauc_numerator(A, Cc, a_neg, c_tot)
        got = fr.sauc_numerator_by_parts(S, pos, neg)
        assert got == want and 0 < want < 2 * a_neg * c_tot, name
        assert fr.sauc_exact(S, pos, neg) == want / (2 * a_neg * c_tot)
    cl = [fr._clamped(pos, neg) for _, _, pos, neg in frames]
    assert max(int(p.max()) for p, _ in cl) == 1023 and max(int(n.max()) for _, n in cl) == 1 << 20
    assert any(len(fr.sauc_points(S, pos, neg)[0]) == 1 for _, S, pos, neg in frames)
    assert any(len(fr.sauc_points(S, pos, neg)[0]) < int((pos > 0).sum()) for _, S, pos, neg in frames)       # tied positives


def test_sauc_exact_halves():
    S, pos, neg = sauc_case(1680, 8, 16)
    assert fr.sauc_exact(np.full((8, 16), 0.25, np.float32), pos, neg) == 0.5          # a constant map
    assert fr.sauc_exact(S, pos, pos) == 0.5                                           # negatives = positives: N = C_tot^2
    assert fr.sauc_exact(fr.quantised(1681, 1, 8, 16)[0], pos, pos) == 0.5
    best = fr.sauc_exact(pos.astype(np.float32), pos, (pos == 0).astype(np.int64))     # the map ranks every positive first
    assert best == 1.0


def test_sauc_degenerate_frames_are_nan():
    S, pos, neg = sauc_case(1690, 8, 16)
    assert math.isnan(fr.sauc_exact(S, np.zeros_like(pos), neg))                       # C_tot = 0
    assert math.isnan(fr.sauc_exact(S, pos, np.zeros_like(neg)))                       # A_neg = 0
    assert math.isnan(fr.sauc_exact(S, -pos, neg))                                     # negative counts clamp to 0
    for bad in (np.nan, np.inf, -np.inf):
        Sb = S.copy()
        Sb[3, 5] = bad
        assert math.isnan(fr.sauc_exact(Sb, pos, neg))
    big_pos, big_neg = np.full((33, 66), 5000, np.int64), np.full((33, 66), 1 << 22, np.int64)      # clamped: 1023 and 2^20
    S33 = hashrng.uniform(1691, (33, 66), 0.0, 1.0, dtype=np.float64).astype(np.float32)
    assert 2 * (33 * 66 * 1023) * (33 * 66 << 20) >= 1 << 53
    assert math.isnan(fr.sauc_exact(S33, big_pos, big_neg))
    big_neg[0, 0] = 0                                                                  # values above the clamp count as the clamp
    assert fr.sauc_points(S33, big_pos, big_neg)[2:] == ((33 * 66 - 1) << 20, 33 * 66 * 1023)
    assert not math.isnan(fr.sauc_exact(S33, big_pos // 5000, big_neg))


def test_shuffled_auc_takes_the_equator_prior_out():
    """A video whose viewers follow per-frame targets drawn from an equator prior.  The map that only says 'look at the horizon'
    must score lower on shuffled AUC (negatives: the other frames' fixations) than the per-frame density does, and lower than
    its own K14 AUC-Judd, whose negatives are every non-fixated pixel.  Measured, means over 8 frames: prior sAUC 0.503, density
    sAUC 0.996, prior AUC-Judd 0.840."""
    F, viewers, h, w = 8, 30, 60, 120
    lonlat, offsets, prior = fr.prior_video(1700, F, viewers, h, w)
    counts, n = fr.bin_points(lonlat, offsets, h, w)
    assert np.all(n == viewers)
    neg = fr.other_frames(counts)
    dens = fr.density64(lonlat, offsets, h, w, np.deg2rad(5.0)).astype(np.float32)
    prior_sauc = np.mean([fr.sauc_exact(prior, counts[f], neg[f]) for f in range(F)])
    dens_sauc = np.mean([fr.sauc_exact(dens[f], counts[f], neg[f]) for f in range(F)])
    a = rs.weights(h)
    prior_judd = np.mean([rs.frame_scores(prior, dens[f], a, counts[f] > 0, exact_auc=True)[0]['auc'] for f in range(F)])
    print('prior sAUC %.4f, density sAUC %.4f, prior AUC-Judd %.4f' % (prior_sauc, dens_sauc, prior_judd))
    assert prior_sauc < dens_sauc and prior_sauc < prior_judd


# ----------------------------------------------------------------------------- scan-paths
def test_slerp_midpoint_across_the_seam_is_on_the_great_circle():
    a_lon, b_lon, lat = np.deg2rad(135.0), np.deg2rad(-135.0), np.deg2rad(30.0)       # 90 degrees of longitude apart, across +-pi
    tracks = [(np.array([0.0, 0.2]), np.array([a_lon, b_lon]), np.array([lat, lat]))]
    for fn in (fr.slerp_points, fixations.scanpaths_to_points):
        lonlat, offsets = fn(tracks, 5.0, 1)                           # frame 0 at t = 0.1: the midpoint
        assert offsets.tolist() == [0, 1] and offsets.dtype == np.int32 and lonlat.dtype == np.float64
        a, b, m = fr.unit(a_lon, lat), fr.unit(b_lon, lat), fr.unit(*lonlat[0])
        assert abs(abs(lonlat[0, 0]) - PI) <= 1e-12                    # on the seam, not at longitude 0
        assert abs(m @ np.cross(a, b)) <= 1e-15 * 10                   # in the plane of the two
        assert abs(m @ a - m @ b) <= 1e-15 * 10 and m @ a > a @ b      # halfway, between them
        assert lonlat[0, 1] > lat                                      # the great circle bulges towards the pole: not the mean latitude


def test_slerp_gaps_spans_and_viewers():
    t = np.array([0.1, 0.3, 1.2, 1.3])                                 # a gap of 0.9 s between 0.3 and 1.2
    one = (t, np.deg2rad([10.0, 20.0, 30.0, 40.0]), np.deg2rad([0.0, 5.0, 10.0, 15.0]))
    two = (np.array([0.25]), np.array([1.0]), np.array([0.5]))         # a single sample: only a frame at that very time
    empty = (np.zeros(0), np.zeros(0), np.zeros(0))
    for fn in (fr.slerp_points, fixations.scanpaths_to_points):
        lonlat, offsets = fn([one, two, empty], 10.0, 15)              # frames at 0.05, 0.15, .., 1.45
        per_frame = np.diff(offsets).tolist()
        assert per_frame == [0, 1, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0], per_frame
        assert np.allclose(lonlat[2], [1.0, 0.5], atol=1e-15)          # frame 2 at 0.25: viewer one, then viewer two on its sample
        wide, offs = fn([one], 10.0, 15, max_gap=1.0)
        assert np.diff(offs).tolist() == [0] + [1] * 12 + [0, 0]
    a = fr.slerp_points([one, two, empty], 10.0, 15)
    b = fixations.scanpaths_to_points([one, two, empty], 10.0, 15)
    assert np.array_equal(a[1], b[1]) and np.allclose(a[0], b[0], rtol=0.0, atol=1e-14)


def test_scanpaths_match_the_restatement_on_random_tracks():
    tracks = []
    for v in range(7):
        n = 20 + 3 * v
        t = np.cumsum(hashrng.uniform(1710 + v, (n,), 0.02, 0.2, dtype=np.float64)) + 0.1 * v
        lon = hashrng.uniform(1720 + v, (n,), -PI, PI, dtype=np.float64)
        lat = hashrng.uniform(1730 + v, (n,), -1.4, 1.4, dtype=np.float64)
        tracks.append((t, lon, lat))
    a = fr.slerp_points(tracks, 30.0, 90, max_gap=0.15)
    b = fixations.scanpaths_to_points(tracks, 30.0, 90, max_gap=0.15)
    assert np.array_equal(a[1], b[1]) and 0 < a[1][-1] < 7 * 90
    assert np.max(np.abs(fr.unit(*a[0].T) - fr.unit(*b[0].T))) <= 1e-13
    with pytest.raises(ValueError):
        fixations.scanpaths_to_points([(np.array([0.2, 0.1]), np.zeros(2), np.zeros(2))], 30.0, 3)
    with pytest.raises(ValueError):
        fixations.scanpaths_to_points(tracks, 0.0, 3)


# ----------------------------------------------------------------------------- library
def test_library_exports_the_symbols():
    L = _lib.lib()
    for name in K15:
        assert name in _lib.PUBLIC_SYMBOLS and hasattr(L, name)
    assert L.cp360_version() == 306


def test_status_codes_without_gpu():
    """Argument validation happens before any launch: the dummy pointers are never used."""
    L = _lib.lib()
    one, big = C.c_void_p(16), 1 << 40
    counts = lambda ll, off, N, F, h, w, c, n: L.cp360_fix_counts(ll, off, N, F, h, w, c, n, None)
    density = lambda ll, off, N, F, h, w, sg, out, wk, nb: L.cp360_fix_density(ll, off, N, F, h, w, sg, out, wk, nb, None)
    sauc = lambda S, p, n, Fn, F, h, w, a, c, an, wk, nb: L.cp360_fix_sauc(S, p, n, Fn, F, h, w, a, c, an, wk, nb, None)
    ok_c = [one, one, 5, 2, 8, 16, one, one]
    ok_d = [one, one, 5, 2, 8, 16, 0.1, one, one, big]
    ok_s = [one, one, one, 2, 2, 8, 16, one, one, one, one, big]
    for fn, ok, ptrs in ((counts, ok_c, (0, 1, 6, 7)), (density, ok_d, (0, 1, 7, 8)), (sauc, ok_s, (0, 1, 2, 7, 8, 9, 10))):
        for k in ptrs:
            args = list(ok)
            args[k] = None
            assert fn(*args) == NULL, (fn, k)
    for F, h, w in ((0, 8, 16), (2, 0, 16), (2, 8, 0), (-1, 8, 16), (2, -8, 16), (2, 8, -16)):
        assert counts(one, one, 5, F, h, w, one, one) == BAD_SHAPE
        assert density(one, one, 5, F, h, w, 0.1, one, one, big) == BAD_SHAPE
        assert sauc(one, one, one, 1, F, h, w, one, one, one, one, big) == BAD_SHAPE
        if F != 0:
            assert L.cp360_fix_work_bytes(F, h, w) == 0
    assert counts(one, one, -1, 2, 8, 16, one, one) == BAD_SHAPE and density(one, one, -1, 2, 8, 16, 0.1, one, one, big) == BAD_SHAPE
    for sg in (0.0, -0.1, float('nan'), float('inf')):
        assert density(one, one, 5, 2, 8, 16, sg, one, one, big) == BAD_SHAPE
    for Fn in (0, 3, -1):
        assert sauc(one, one, one, Fn, 2, 8, 16, one, one, one, one, big) == BAD_SHAPE
    for F, h, w in ((65536, 8, 16), (1, 1024, 2049)):
        assert counts(one, one, 5, F, h, w, one, one) == UNSUPPORTED
        assert density(one, one, 5, F, h, w, 0.1, one, one, big) == UNSUPPORTED
        assert sauc(one, one, one, 1, F, h, w, one, one, one, one, big) == UNSUPPORTED
        assert L.cp360_fix_work_bytes(F, h, w) == 0
    assert counts(one, one, 1 << 31, 2, 8, 16, one, one) == UNSUPPORTED and density(one, one, 1 << 31, 2, 8, 16, 0.1, one, one, big) == UNSUPPORTED
    assert L.cp360_fix_work_bytes(1, 1024, 2048) > 0 and L.cp360_fix_work_bytes(0, 1024, 2049) == 0
    tables, need = L.cp360_fix_work_bytes(0, 8, 16), L.cp360_fix_work_bytes(2, 8, 16)
    assert tables % 16 == 0 and tables >= (8 + 16) * 8 and need % 16 == 0 and need >= tables + 2 * 8 * 16 * 8
    assert density(one, one, 5, 2, 8, 16, 0.1, one, one, tables - 1) == BAD_SHAPE      # workspace too small
    assert sauc(one, one, one, 1, 2, 8, 16, one, one, one, one, need - 1) == BAD_SHAPE
    assert counts(C.c_void_p(4), one, 5, 2, 8, 16, one, one) == ALIGN and counts(one, C.c_void_p(2), 5, 2, 8, 16, one, one) == ALIGN
    assert counts(one, one, 5, 2, 8, 16, C.c_void_p(2), one) == ALIGN
    assert density(one, one, 5, 2, 8, 16, 0.1, one, C.c_void_p(8), big) == ALIGN and density(one, one, 5, 2, 8, 16, 0.1, C.c_void_p(2), one, big) == ALIGN
    assert sauc(one, one, one, 1, 2, 8, 16, C.c_void_p(4), one, one, one, big) == ALIGN
    assert sauc(one, one, one, 1, 2, 8, 16, one, one, one, C.c_void_p(8), big) == ALIGN
    assert sauc(C.c_void_p(2), one, one, 1, 2, 8, 16, one, one, one, one, big) == ALIGN


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    lonlat, offsets = torch.zeros(4, 2, dtype=torch.float64), torch.tensor([0, 4], dtype=torch.int32)
    S, pos = torch.zeros(1, 8, 16), torch.zeros(1, 8, 16, dtype=torch.int32)
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.fixation_counts(lonlat, offsets, (8, 16))
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.fixation_density(lonlat, offsets, (8, 16), 0.1)
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.shuffled_auc(S, pos, pos)
    with pytest.raises(ValueError):
        fixations.FixationMaps(grid_hw=(0, 16))
    with pytest.raises(ValueError):
        fixations.FixationMaps(grid_hw=(1024, 2049))
    with pytest.raises(ValueError):
        fixations.FixationMaps(sigma_deg=0.0)
    with pytest.raises(ValueError):
        fixations.save_gt('/nonexistent', 'v', np.zeros((8, 16), np.float32))
