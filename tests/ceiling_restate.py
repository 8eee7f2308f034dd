"""Numpy restatement of the point scores behind the human ceiling and the prior baselines (K19, csrc/fixations.hip; the
specification is DESIGN.md "K19"), on top of tests/fixations_restate.py (the binning, the density terms, the synthetic points)
and tests/sphere_eval_restate.py (the row weights): float64 sums by numpy and exact Python integers for the AUC, and the cases
that the CPU and GPU tests share.  Not a test file.

    points   K15's CSR points; the points of one frame are taken as different viewers'; point k of frame f lies in pixel i_k
    l_k      leave-one-out: max(T_f - e_k, 0), T_f = sum_k e_k over the frame's finite points in ascending k, e_k[j] = exp(kappa
             (p_j . q_k - 1));  map mode: S[f] (or S[0])
    nss      (l_k[i_k] - mu) / sigma,  mu = sum_a l_k / A,  sigma = sqrt(sum_a (l_k - mu)^2 / A)
    auc      1 - A_k / (2 A_neg) = (2 A_neg - A_k) / (2 A_neg),  A_k = sum of a_j over j != i_k with l_k[j] >= l_k[i_k],  A_neg = A -
             a_{i_k}: K14's AUC-Judd with the one fixated pixel i_k
    NaN      a point with a non-finite coordinate or outside every frame: both;  a non-finite value in the frame's S: both
"""
import functools

import numpy as np

from tests import fixations_restate as fr
from tests import sphere_eval_restate as rs
from tests.test_fixations_gpu import DENSITY_GATE

MAX_WEIGHT = 1024
NAN = float('nan')


# ----------------------------------------------------------------------------- the points
def pixel_weights(h, w, a_rows):
    """int64 [h w]: the weight of every pixel, its row's, clamped to 0 .. 1024 as K14 clamps it."""
    return np.repeat(np.clip(np.asarray(a_rows, np.int64), 0, MAX_WEIGHT), w)


def _alone(n):
    return np.arange(n + 1)                                            # every point a frame of its own


def point_pixels(lonlat, h, w):
    """-> (finite bool [N], pixel int64 [N]): fixations_restate.bin_points of every point alone; 0 for a dropped point."""
    lonlat = np.asarray(lonlat, np.float64).reshape(-1, 2)
    counts, n = fr.bin_points(lonlat, _alone(len(lonlat)), h, w)
    return n > 0, counts.reshape(len(lonlat), -1).argmax(axis=1)


def frame_ranges(offsets, N):
    """The points of every frame as K15 clamps them: [(k0, k1)]."""
    out = []
    for f in range(len(offsets) - 1):
        k0 = min(max(int(offsets[f]), 0), N)
        out.append((k0, min(max(int(offsets[f + 1]), k0), N)))
    return out


def point_terms(lonlat, h, w, sigma_rad, f32_terms=False):
    """float64 [N, h w]: e_k, the density of point k alone - fixations_restate.density64, or density32 (the kernel's f32
    operations in its order) widened; zeros for a dropped point."""
    lonlat = np.asarray(lonlat, np.float64).reshape(-1, 2)
    e = (fr.density32 if f32_terms else fr.density64)(lonlat, _alone(len(lonlat)), h, w, sigma_rad)
    return np.asarray(e, np.float64).reshape(len(lonlat), -1)


def loo_maps(lonlat, offsets, h, w, sigma_rad, f32_terms=False):
    """-> (l float64 [N, h w], T float64 [F, h w]): the leave-one-out map of every point (a row of NaN for a point without one)
    and the frames' totals, added in ascending k."""
    lonlat = np.asarray(lonlat, np.float64).reshape(-1, 2)
    N = len(lonlat)
    e = point_terms(lonlat, h, w, sigma_rad, f32_terms)
    finite = point_pixels(lonlat, h, w)[0]
    l = np.full((N, h * w), NAN)
    T = np.zeros((len(offsets) - 1, h * w))
    for f, (k0, k1) in enumerate(frame_ranges(offsets, N)):
        for k in range(k0, k1):
            T[f] = T[f] + e[k]
        for k in range(k0, k1):
            if finite[k]:
                l[k] = np.maximum(T[f] - e[k], 0.0)
    return l, T


# ----------------------------------------------------------------------------- the scores of one point
def point_score(l, i, a):
    """l float64 [P], the point's pixel i, a int64 [P] -> (auc, nss, A_k, A_neg): the AUC one quotient of Python integers."""
    l = np.asarray(l, np.float64).reshape(-1)
    if not np.all(np.isfinite(l)):
        return NAN, NAN, 0, 0
    A = int(a.sum())
    with np.errstate(all='ignore'):
        mu = (a * l).sum() / np.float64(A)
        sigma = np.sqrt((a * (l - mu) ** 2).sum() / np.float64(A))
        nss = float((l[i] - mu) / sigma)
    ge = l >= l[i]
    ge[i] = False
    A_k, A_neg = int(a[ge].sum()), A - int(a[i])
    return ((2 * A_neg - A_k) / (2 * A_neg) if A_neg else NAN), nss, A_k, A_neg


def point_band(l, T, i, a, rel):
    """The comparisons of one leave-one-out point that rel cannot decide: |l[j] - l[i]| <= rel (l[j] + l[i]) + 2^-50 (T[j] +
    T[i]) -> (auc with them counted in, auc with them counted out, their weight, the weight of all comparisons = A_neg)."""
    und = np.abs(l - l[i]) <= rel * (l + l[i]) + 2.0 ** -50 * (T + T[i])
    und[i] = False
    ge = (l >= l[i]) & ~und
    ge[i] = False
    A_neg = int(a.sum()) - int(a[i])
    lo, u = int(a[ge].sum()), int(a[und].sum())
    if A_neg == 0:
        return NAN, NAN, 0, 0
    return (2 * A_neg - (lo + u)) / (2 * A_neg), (2 * A_neg - lo) / (2 * A_neg), u, A_neg


# ----------------------------------------------------------------------------- the scores of a video
def loo_scores(lonlat, offsets, h, w, sigma_rad, a_rows, f32_terms=False, rel=None):
    """-> {'auc', 'nss' float64 [N]} and, with rel, {'auc_lo', 'auc_hi' float64 [N], 'undecided', 'compared' int64 [N]}."""
    lonlat = np.asarray(lonlat, np.float64).reshape(-1, 2)
    N = len(lonlat)
    a = pixel_weights(h, w, a_rows)
    l, T = loo_maps(lonlat, offsets, h, w, sigma_rad, f32_terms)
    pix = point_pixels(lonlat, h, w)[1]
    out = {k: np.full(N, NAN) for k in ('auc', 'nss', 'auc_lo', 'auc_hi')}
    out.update({k: np.zeros(N, np.int64) for k in ('undecided', 'compared')})
    for f, (k0, k1) in enumerate(frame_ranges(offsets, N)):
        for k in range(k0, k1):
            if np.isnan(l[k, 0]):
                continue
            out['auc'][k], out['nss'][k] = point_score(l[k], pix[k], a)[:2]
            if rel is not None:
                out['auc_lo'][k], out['auc_hi'][k], out['undecided'][k], out['compared'][k] = point_band(l[k], T[f], pix[k], a, rel)
    return out


def map_scores(S, lonlat, offsets, h, w, a_rows):
    """S [1 or F, h, w] -> (auc, nss float64 [N]): every point of frame f against S[f] (or S[0])."""
    lonlat = np.asarray(lonlat, np.float64).reshape(-1, 2)
    N = len(lonlat)
    a = pixel_weights(h, w, a_rows)
    finite, pix = point_pixels(lonlat, h, w)
    auc, nss = np.full(N, NAN), np.full(N, NAN)
    for f, (k0, k1) in enumerate(frame_ranges(offsets, N)):
        l = np.asarray(S[f if len(S) > 1 else 0], np.float64).reshape(-1)
        for k in range(k0, k1):
            if finite[k]:
                auc[k], nss[k] = point_score(l, pix[k], a)[:2]
    return auc, nss


def video_means(v, offsets):
    """v float64 [N] -> (the frames' means over their points that have a number, NaN for a frame with none; the video's)."""
    with np.errstate(all='ignore'):
        fm = np.array([np.nanmean(v[k0:k1]) if np.any(~np.isnan(v[k0:k1])) else NAN for k0, k1 in frame_ranges(offsets, len(v))])
        return fm, float(np.nanmean(v)) if np.any(~np.isnan(v)) else NAN


# ----------------------------------------------------------------------------- the shared cases
# The density gate of tests/test_fixations_gpu.py per sigma (four times the larger measured error of a density against float64,
# in units of the maximum): the relative error that a leave-one-out map may carry, and so the band within which a comparison
# of two of its values is undecided.  10 degrees has no gate of its own: the error falls with sigma, so 5 degrees' holds.
DENSITY_REL = dict(DENSITY_GATE)
DENSITY_REL[10.0] = DENSITY_REL[5.0]

# name: (h, w, sigma_deg, weights, the points of every frame): fixations_restate.prior_video(1900, ..), viewers around a target
LOO_CASES = {
    'wave': (5, 9, 20.0, 'solid_angle', [12] * 4),                     # P = 45: fewer pixels than a wave has lanes
    'small': (12, 24, 20.0, 'solid_angle', [12] * 5),
    'mid5': (30, 60, 5.0, 'solid_angle', [12] * 6),
    'mid10': (30, 60, 10.0, 'solid_angle', [12] * 6),
    'odd': (33, 66, 5.0, 'solid_angle', [70] * 3),                     # P no multiple of 256, 70 points cross a 64-point tile
    'full': (120, 240, 5.0, 'solid_angle', [30] * 2),
    'frames': (30, 60, 10.0, 'solid_angle', [0, 1, 2, 64, 65, 300]),   # 300 crosses the 256-point staging tile
    'uniform': (12, 24, 20.0, 'uniform', [12] * 5),
    'twins': (30, 60, 10.0, 'solid_angle', [12]),                      # and two more: point 0 again, the centre of point 1's pixel
}


@functools.lru_cache(maxsize=None)
def loo_case(name):
    """-> (lonlat, offsets, a_rows int64 [h]), read-only: every frame keeps the first of prior_video's viewers."""
    h, w, _, mode, per_frame = LOO_CASES[name]
    lonlat, offsets, _ = fr.prior_video(1900, len(per_frame), max(per_frame), h, w)
    keep = np.concatenate([np.arange(offsets[f], offsets[f] + n) for f, n in enumerate(per_frame)]).astype(np.int64)
    lonlat = np.ascontiguousarray(lonlat[keep])
    offsets = np.concatenate([[0], np.cumsum(per_frame)]).astype(np.int32)
    if name == 'twins':
        pix = point_pixels(lonlat[1:2], h, w)[1][0]
        centre = [((2.0 * (pix % w) + 1.0) / w - 1.0) * np.pi, (1.0 - (2.0 * (pix // w) + 1.0) / h) * (np.pi / 2.0)]
        lonlat, offsets = np.ascontiguousarray(np.concatenate([lonlat, lonlat[:1], [centre]])), np.array([0, 14], np.int32)
    a_rows = rs.weights(h, mode)
    for v in (lonlat, offsets, a_rows):
        v.setflags(write=False)
    return lonlat, offsets, a_rows


@functools.lru_cache(maxsize=None)
def loo_case_scores(name, f32_terms=False):
    """The restated scores of a case, with the undecided band of its sigma's gate; computed once."""
    h, w, sigma_deg, _, _ = LOO_CASES[name]
    lonlat, offsets, a_rows = loo_case(name)
    out = loo_scores(lonlat, offsets, h, w, np.deg2rad(sigma_deg), a_rows, f32_terms, DENSITY_REL[sigma_deg])
    for v in out.values():
        v.setflags(write=False)
    return out
