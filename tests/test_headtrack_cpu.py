"""Head-tracking ground truth (K17) without a GPU: the host interpolation of the head logs (utils/headtrack.py: head_cameras),
the claims of the restatement (tests/headtrack_restate.py) that tests/test_headtrack_gpu.py holds the kernels to - with the cap
on what float32 cannot decide asserted for every GPU case - and the library's exports and status codes."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from cp_360_weakly_supervised_saliency_amd import _lib, ops
from cp_360_weakly_supervised_saliency_amd.utils import fixations, hashrng, headtrack, viewport
from tests import headtrack_restate as hr
from tests import viewport_restate as vr

K17 = ('cp360_head_footprints', 'cp360_head_agreement')
NULL, BAD_SHAPE, ALIGN, UNSUPPORTED = -5, -1, -6, -8
PI = math.pi


# ----------------------------------------------------------------------------- head_cameras
def tracks7(roll=False):
    """Seven viewers, 3 s at 10 Hz: smooth random walks; one with a gap, one short, one with a NaN sample, one empty."""
    tracks = []
    for v in range(7):
        t = np.arange(31) * 0.1
        lon = np.cumsum(0.2 * hashrng.normal(300 + v, (31,), dtype=np.float64)) + v
        lat = np.clip(np.cumsum(0.1 * hashrng.normal(310 + v, (31,), dtype=np.float64)), -1.5, 1.5)
        r = np.cumsum(0.3 * hashrng.normal(320 + v, (31,), dtype=np.float64))
        if v == 1:
            t = np.concatenate([t[:10], t[10:] + 0.7])                 # a gap of 0.8 s
        if v == 2:
            t, lon, lat, r = t[5:20], lon[5:20], lat[5:20], r[5:20]    # a span of 0.5 .. 1.9 s
        if v == 3:
            lon[12] = np.nan
        if v == 4:
            t, lon, lat, r = t[:0], lon[:0], lat[:0], r[:0]
        tracks.append((t, lon, lat, r) if roll else (t, lon, lat))
    return tracks


def test_directions_are_scanpaths_to_points():
    tracks = tracks7()
    lonlat, offsets = fixations.scanpaths_to_points(tracks, 30.0, 100, max_gap=0.5)
    R, off, viewer = headtrack.head_cameras(tracks, 30.0, 100, max_gap=0.5)
    assert R.dtype == np.float32 and off.dtype == np.int32 and viewer.dtype == np.int32
    assert np.array_equal(off, offsets) and R.shape == (int(offsets[-1]), 3, 3) and viewer.shape == (R.shape[0],)
    cl = np.cos(lonlat[:, 1])
    want = np.stack([cl * np.cos(lonlat[:, 0]), np.sin(lonlat[:, 1]), cl * np.sin(lonlat[:, 0])], -1)
    assert np.max(np.abs(R[:, :, 0] - want)) <= 2.0 ** -23           # the same float64 direction, rounded to float32 once
    # the drop rules, through the viewer indices: nobody past 3 s or 3.7 s, the gap, the span, the NaN sample's two intervals
    tf = (np.arange(100) + 0.5) / 30.0
    frame = np.searchsorted(off[1:], np.arange(R.shape[0]), side='right')
    seen = lambda v: set(frame[viewer == v].tolist())
    assert seen(0) == set(np.flatnonzero(tf <= 3.0).tolist())
    assert seen(1) == set(np.flatnonzero(((tf <= 0.9) | (tf >= 1.7)) & (tf <= 3.7)).tolist())
    assert seen(2) == set(np.flatnonzero((tf >= 0.5) & (tf <= 1.9)).tolist())
    assert seen(3) == set(np.flatnonzero(((tf <= 1.1) | (tf >= 1.3)) & (tf <= 3.0)).tolist())
    assert seen(4) == set() and seen(5) == seen(0) == seen(6)
    for f in range(100):                                               # frame by frame, viewers in their order
        assert np.all(np.diff(viewer[off[f]:off[f + 1]]) > 0)
    tight = headtrack.head_cameras(tracks, 30.0, 100, max_gap=0.05)    # every interval is 0.1 s: only frames on a sample stay
    assert tight[1][-1] < off[-1] // 4


def test_cameras_are_look_at_rolled_and_orthonormal():
    flat = headtrack.head_cameras(tracks7(), 30.0, 100)
    R, off, viewer = headtrack.head_cameras(tracks7(roll=True), 30.0, 100)
    assert np.array_equal(off, flat[1]) and np.array_equal(viewer, flat[2])
    assert np.max(np.abs(np.einsum('nij,nik->njk', R.astype(np.float64), R.astype(np.float64)) - np.eye(3))) <= 1e-6
    assert np.max(np.abs(np.linalg.det(R.astype(np.float64)) - 1.0)) <= 1e-6
    assert np.array_equal(R[:, :, 0], flat[0][:, :, 0])               # the roll leaves the forward axis alone
    for k in range(0, R.shape[0], 37):                                 # without roll: look_at itself, a level horizon
        want = viewport.look_at(flat[0][k, :, 0].astype(np.float64))
        assert np.max(np.abs(flat[0][k] - want)) <= 1e-6 and abs(float(flat[0][k, 1, 2])) <= 1e-6
    # the roll angle, read back from the rolled up axis in the level camera's (up, right) basis
    t, lon, lat, r = tracks7(roll=True)[0]
    tf = (np.arange(100) + 0.5) / 30.0
    keep = viewer == 0
    got = np.arctan2(np.einsum('ni,ni->n', R[keep][:, :, 1], flat[0][keep][:, :, 2]),
                     np.einsum('ni,ni->n', R[keep][:, :, 1], flat[0][keep][:, :, 1]))
    want = np.interp(tf[:int(keep.sum())], t, r)                       # its steps are far below pi: plain linear interpolation
    assert np.max(np.abs(np.angle(np.exp(1j * (got - want))))) <= 1e-5


def test_roll_wraps_the_short_way_and_poles_chain():
    t = np.array([0.0, 1.0])
    zero = np.zeros(2)
    R, off, _ = headtrack.head_cameras([(t, zero, zero, np.array([3.0, -3.0]))], 4.0, 4, max_gap=1.0)      # 3 -> -3: 0.283 rad through pi
    assert off.tolist() == [0, 1, 2, 3, 4]
    got = np.arctan2(R[:, 2, 1], R[:, 1, 1])                          # forward (1, 0, 0), up (0, 1, 0), right (0, 0, 1)
    want = 3.0 + (np.arange(4) + 0.5) / 4.0 * (2.0 * PI - 6.0)
    assert np.max(np.abs(np.angle(np.exp(1j * (got - want))))) <= 1e-6
    # a viewer who looks over the north pole: at the pole the right of the frame before is kept
    lat = np.array([PI / 2 - 0.2, PI / 2, PI / 2 - 0.2])
    R, off, _ = headtrack.head_cameras([(np.array([0.5, 1.5, 2.5]), np.array([0.3, 0.3, 0.3 + PI]), lat)], 1.0, 3, max_gap=2.0)
    assert off.tolist() == [0, 1, 2, 3] and abs(float(R[1, 1, 0]) - 1.0) <= 1e-7          # the second frame sits on the pole's sample
    chain = vr.cameras(R[:, :, 0].astype(np.float64))
    assert np.max(np.abs(R - chain)) <= 1e-6 and np.max(np.abs(R[1, :, 2] - R[0, :, 2])) <= 1e-6 and float(R[2, :, 2] @ R[0, :, 2]) < -0.99
    R, off, _ = headtrack.head_cameras([(np.array([0.0, 2.0]), zero, np.array([PI / 2, PI / 2]))], 1.0, 2, max_gap=2.0)
    assert off.tolist() == [0, 1, 2] and np.max(np.abs(R[0] - vr.look_at([0.0, 1.0, 0.0]))) <= 1e-6 and np.max(np.abs(R[0] - R[1])) <= 1e-6
    with pytest.raises(ValueError):
        headtrack.head_cameras([(t, zero)], 4.0, 4)
    with pytest.raises(ValueError):
        headtrack.head_cameras([(t, zero, zero, np.zeros(3))], 4.0, 4)
    with pytest.raises(ValueError):
        headtrack.head_cameras([(t, zero, zero)], 0.0, 4)
    none = headtrack.head_cameras([], 4.0, 3)
    assert none[0].shape == (0, 3, 3) and none[1].tolist() == [0, 0, 0, 0] and none[2].shape == (0,)


# ----------------------------------------------------------------------------- the restatement
def test_inside_is_the_area_that_outline_encloses():
    """The border that K12b draws lies inside the footprint and the footprint's outermost pixels lie on it."""
    R = vr.rot([0.3, 1.0, -0.2], 0.9)
    for view in (hr.VIEW_A, hr.VIEW_B):
        m = hr.inside(R, 60, 120, view)[0]
        border = vr.outline(R, 60, 120, view[0], view[1], border_px=1)[0]
        assert m.any() and border.any() and not (border & ~m).any()
        assert hr.tangents(view, np.float32) == vr.view_tangents(view[0], view[1], np.float32)         # K12b's thresholds, bit for bit
        assert abs(hr.tangents(view)[1] - vr.view_tangents(*view)[1]) <= 2.0 ** -52 * hr.tangents(view)[1]


@pytest.mark.parametrize('lat_deg', [0.0, 60.0, 90.0])
def test_footprint_area_is_the_solid_angle_of_the_view(lat_deg):
    """The solid angle of a rectangular window with the half-angles' tangents tx, ty is 4 asin(tx ty / sqrt((1 + tx^2)(1 + ty^2))).
    The weighted pixel count differs from it by the pixels that the edge cuts - at most the weight of the footprint's own edge
    pixels and as much outside - and by the rounding of the weights to 1 / 1024 (at most 1 / 2048 of a pixel's area each)."""
    h, w = 120, 240
    a = hr.row_weights(h, 'solid_angle')
    px_area = (PI / h) * (2.0 * PI / w) / 1024.0
    R = vr.look_at([math.cos(math.radians(lat_deg)) * math.cos(0.4), math.sin(math.radians(lat_deg)), math.cos(math.radians(lat_deg)) * math.sin(0.4)])
    for view in (((1, 1), 100.0), hr.VIEW_A):
        tx, ty = hr.tangents(view)
        omega = 4.0 * math.asin(tx * ty / math.sqrt((1.0 + tx * tx) * (1.0 + ty * ty)))
        m = hr.inside(R, h, w, view)[0]
        nb = np.roll(m, 1, 1) & np.roll(m, -1, 1) & np.vstack([m[:1], m[:-1]]) & np.vstack([m[1:], m[-1:]])
        edge = float((a[:, None] * (m & ~nb)).sum()) * px_area
        got = float((a[:, None] * m).sum()) * px_area
        assert abs(got - omega) <= 2.0 * edge + m.sum() * px_area * 0.5, (view, got, omega, edge)
        assert abs(got - omega) <= 0.1 * omega


def test_restatement_identities():
    c = hr.case('gaps_30x60')
    (h, w), R, off, view, a = c['grid'], c['R'], c['offsets'], c['view'], c['weights']
    counts, n_views = hr.footprints(R, off, h, w, view)
    assert n_views.tolist() == [19, 0, 29, 20, 0] and counts[1].sum() == 0 == counts[4].sum()
    assert np.array_equal(counts.sum(axis=0), c['ins'].sum(axis=0))
    one = np.arange(len(R) + 1)
    own = hr.agreement(R, view, R, one, h, w, view, a)                 # every viewer against itself
    assert np.array_equal(own[0], own[1]) and own[0][3] == 0 == own[0][25] and own[0][7] > 0 and own[0][55] > 0
    for f in range(5):
        assert int((a[:, None] * counts[f]).sum()) == int(own[0][off[f]:off[f + 1]].sum())
    inter, uni = hr.agreement(c['Rc'], c['cam_view'], R, off, h, w, view, a)
    assert np.all(inter <= uni) and np.all(inter >= 0)
    assert inter[3] == 0 == inter[25] and uni[3] == (a[:, None] * c['cins'][0]).sum() and uni[25] == (a[:, None] * c['cins'][2]).sum()
    assert np.all(inter[50:] == 0) and np.array_equal(uni[50:], own[0][50:])          # the fourth frame's camera is not finite
    flip = R.astype(np.float64) * np.array([-1.0, 1.0, -1.0])         # half a turn about up: the view behind
    sq = ((1, 1), 90.0)
    back = hr.agreement(flip, sq, R, one, h, w, sq, a)
    area = hr.agreement(R, sq, R, one, h, w, sq, a)[0]
    area_back = hr.agreement(flip, sq, flip, one, h, w, sq, a)[0]
    assert np.all(back[0] == 0) and np.array_equal(back[1], area + area_back)
    assert hr.frame_of([0, 0, 2, 2, 3], 3).tolist() == [1, 1, 3]


@pytest.mark.parametrize('name', sorted(hr.CASES))
def test_float32_decides_all_but_a_thousandth(name):
    """The cap of the GPU tests, from the reference alone: the pairs float32 cannot decide are at most 0.1 % of the inside ones."""
    c = hr.case(name)
    for ins, und, what in ((c['ins'], c['und'], 'viewers'), (c['cins'], c['cund'], 'cameras')):
        n_in, n_und = int(ins.sum()), int(und.sum())
        print('%s %s: %d cameras, %d inside pairs, %d undecided' % (name, what, len(ins), n_in, n_und))
        assert n_und <= 0.001 * n_in
    lo, hi = hr.count_bounds(c)
    c32 = hr.footprints(c['R'], c['offsets'], c['grid'][0], c['grid'][1], c['view'], np.float32)[0]
    assert np.all(lo <= c32) and np.all(c32 <= hi)                     # the float32 restatement keeps the bound it sets
    b = hr.agreement_bounds(c)
    i32, u32 = hr.agreement(c['Rc'], c['cam_view'], c['R'], c['offsets'], c['grid'][0], c['grid'][1], c['view'], c['weights'], np.float32)
    assert np.all(b[0] <= i32) and np.all(i32 <= b[1]) and np.all(b[2] <= u32) and np.all(u32 <= b[3])
    if name == 'narrow_5x9':
        # a window smaller than a pixel: its diagonal, 14.1 degrees, is below twice the least distance of two pixel centres
        # (12.4 degrees, in the rows next to the poles), so it holds two centres at the most
        assert int(c['ins'].sum(axis=(1, 2)).max()) <= 2 and not c['ins'].all(axis=0).any()
    if name == 'wide_5x9':
        assert c['ins'].sum() > 0.4 * c['ins'].size


# ----------------------------------------------------------------------------- library
def test_library_exports_the_symbols():
    L = _lib.lib()
    for name in K17:
        assert name in _lib.PUBLIC_SYMBOLS and hasattr(L, name)
    assert L.cp360_version() == 306


def test_status_codes_without_gpu():
    """Argument validation happens before any launch: the dummy pointers are never used."""
    L = _lib.lib()
    one, big = C.c_void_p(16), 1 << 40
    foot = lambda R, off, N, F, h, w, fov, asp, c, n, wk, nb: L.cp360_head_footprints(R, off, N, F, h, w, fov, asp, c, n, wk, nb, None)
    agree = lambda Rc, cf, ca, R, off, N, F, h, w, fov, asp, a, i, u, wk, nb: \
        L.cp360_head_agreement(Rc, cf, ca, R, off, N, F, h, w, fov, asp, a, i, u, wk, nb, None)
    ok_f = [one, one, 5, 2, 8, 16, 1.7, 1.0, one, one, one, big]
    ok_a = [one, 1.5, 0.5625, one, one, 5, 2, 8, 16, 1.7, 1.0, one, one, one, one, big]

    def bad(fn, ok, **kw):
        args = list(ok)
        for k, v in kw.items():
            args[int(k[1:])] = v
        return fn(*args)
    for k in (0, 1, 8, 9, 10):
        assert bad(foot, ok_f, **{'a%d' % k: None}) == NULL, k
    for k in (0, 3, 4, 11, 12, 13, 14):
        assert bad(agree, ok_a, **{'a%d' % k: None}) == NULL, k
    for F, h, w in ((0, 8, 16), (2, 0, 16), (2, 8, 0), (-1, 8, 16), (2, -8, 16), (2, 8, -16)):
        assert bad(foot, ok_f, a3=F, a4=h, a5=w) == BAD_SHAPE and bad(agree, ok_a, a6=F, a7=h, a8=w) == BAD_SHAPE
    assert bad(foot, ok_f, a2=-1) == BAD_SHAPE and bad(agree, ok_a, a5=-1) == BAD_SHAPE
    for fov in (0.0, -0.5, PI, 4.0, float('nan'), float('inf')):
        assert bad(foot, ok_f, a6=fov) == BAD_SHAPE and bad(agree, ok_a, a9=fov) == BAD_SHAPE and bad(agree, ok_a, a1=fov) == BAD_SHAPE
    for asp in (0.0, -1.0, float('nan'), float('inf'), 1e39):          # tan(0.85) 1e39 is not finite in float32
        assert bad(foot, ok_f, a7=asp) == BAD_SHAPE and bad(agree, ok_a, a10=asp) == BAD_SHAPE and bad(agree, ok_a, a2=asp) == BAD_SHAPE
    for F, h, w in ((65536, 8, 16), (1, 1024, 2049)):
        assert bad(foot, ok_f, a3=F, a4=h, a5=w) == UNSUPPORTED and bad(agree, ok_a, a6=F, a7=h, a8=w) == UNSUPPORTED
    assert bad(foot, ok_f, a2=1 << 31) == UNSUPPORTED and bad(agree, ok_a, a5=1 << 31) == UNSUPPORTED
    tables = L.cp360_fix_work_bytes(0, 8, 16)
    assert tables % 16 == 0 and tables >= (8 + 16) * 8
    assert bad(foot, ok_f, a11=tables - 1) == BAD_SHAPE and bad(agree, ok_a, a15=tables - 1) == BAD_SHAPE       # workspace too small
    assert bad(agree, ok_a, a5=0, a15=tables - 1) == BAD_SHAPE and bad(agree, ok_a, a5=0, a3=None, a12=None, a13=None, a15=tables) == 0
    assert bad(foot, ok_f, a10=C.c_void_p(8)) == ALIGN and bad(agree, ok_a, a14=C.c_void_p(8)) == ALIGN
    for k in (0, 1, 8, 9):
        assert bad(foot, ok_f, **{'a%d' % k: C.c_void_p(18)}) == ALIGN, k
    for k in (0, 3, 4, 11):
        assert bad(agree, ok_a, **{'a%d' % k: C.c_void_p(18)}) == ALIGN, k
    for k in (12, 13):
        assert bad(agree, ok_a, **{'a%d' % k: C.c_void_p(20)}) == ALIGN, k


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    R, offsets = torch.zeros(4, 3, 3), torch.tensor([0, 4], dtype=torch.int32)
    a = torch.full((8,), 1024, dtype=torch.int32)
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.head_footprints(R, offsets, (8, 16), (1, 1), 100.0)
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.head_agreement(R[:1], ((9, 16), 90.0), R, offsets, (8, 16), ((1, 1), 100.0), a)
    with pytest.raises(RuntimeError, match='GPU only'):
        headtrack.HeadMaps(device='cpu').footprints(R, offsets)
    for view_hw, fov in (((0, 1), 100.0), ((1, -1), 100.0), ((1, 1), 0.0), ((1, 1), 180.0), ((1, 1), float('nan'))):
        with pytest.raises(ValueError):
            ops._head_view(view_hw, fov)
        with pytest.raises(ValueError):
            headtrack.HeadMaps(view_hw=view_hw, hfov_deg=fov)
    assert ops._head_view((9, 16), 90.0) == (PI / 2, 0.5625)
    with pytest.raises(ValueError):
        headtrack.HeadMaps(grid_hw=(0, 16))
    with pytest.raises(ValueError):
        headtrack.HeadMaps(grid_hw=(1024, 2049))
