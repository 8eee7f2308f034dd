"""Viewport-adaptive streaming (K24) without a GPU: the gaze cameras, the claims of the restatement (tests/streaming_restate.py)
that tests/test_streaming_gpu.py holds the kernels to - with the cap on what float32 cannot decide asserted for every GPU case -
the host side of the planner (segments, the allocation, the uniform plan), and the library's exports, status codes and refusals."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from cp_360_weakly_supervised_saliency_amd import _lib, ops
from cp_360_weakly_supervised_saliency_amd.utils import streaming
from tests import headtrack_restate as hr
from tests import streaming_restate as sr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K24 = ('cp360_view_incidence', 'cp360_tile_incidence', 'cp360_view_expect', 'cp360_view_quality', 'cp360_view_quality_work_bytes')
NULL, BAD_SHAPE, ALIGN, UNSUPPORTED = -5, -1, -6, -8


# ----------------------------------------------------------------------------- gaze cameras
@pytest.mark.parametrize('src', [(2, 4), (7, 14), (14, 28), (3, 5)])
def test_gaze_cameras(src):
    cams = streaming.gaze_cameras(src)
    assert cams.dtype == np.float32 and cams.shape == (src[0] * src[1], 3, 3) and cams.flags['C_CONTIGUOUS']
    c64 = cams.astype(np.float64)
    assert np.max(np.abs(np.einsum('nij,nik->njk', c64, c64) - np.eye(3))) <= 1e-6              # orthonormal
    assert np.all(cams[:, 1, 2] == 0.0)                                                          # level: right_y = 0
    want = sr.pixel_dirs(src)
    assert np.max(np.abs(cams[:, :, 0] - want)) <= 2.0 ** -24                                    # forward: one float32 rounding
    assert np.max(np.abs(cams.astype(np.float64) - sr.cameras(src))) <= 2.0 ** -23               # the restatement's own
    assert np.all(np.linalg.det(c64) > 0.999)
    with pytest.raises(ValueError):
        streaming.gaze_cameras((0, 4))
    with pytest.raises(ValueError):
        streaming.gaze_cameras((64, 65))


# ----------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize('name', sorted(sr.CASES))
def test_float32_decides_all_but_a_thousandth(name):
    """The cap of the GPU tests, from the reference alone: the undecided (camera, pixel) pairs are at most 0.1 % of the inside
    ones, and the float32 restatement of the decision stays between the bounds that it sets."""
    c = sr.case(name)
    n_in, n_und = int(c['ins'].sum()), int(c['und'].sum())
    print('%s: %d cameras, %d inside pairs, %d undecided' % (name, len(c['cams']), n_in, n_und))
    assert n_in > 0 and n_und <= 0.001 * n_in
    m32 = hr.masks(c['cams'], c['grid'][0], c['grid'][1], c['view'], np.float32).reshape(len(c['cams']), -1)
    assert not ((m32 != c['ins']) & ~c['und']).any()


def test_bits_round_trip():
    b = np.zeros((3, 45), bool)
    b[0, [0, 31, 32, 44]] = True
    b[2] = True
    w = sr.pack_bits(b)
    assert w.dtype == np.uint32 and w.shape == (3, 2)
    assert w[0].tolist() == [0x80000001, (1 << 12) | 1] and w[1].tolist() == [0, 0] and w[2].tolist() == [0xffffffff, (1 << 13) - 1]
    assert np.array_equal(sr.unpack_bits(w, 45), b) and np.array_equal(sr.unpack_bits(w.view(np.int32), 45), b)


def test_tiles_of_an_uneven_division():
    idx = sr.tile_index((5, 9), (2, 3)).reshape(5, 9)
    assert idx[:, 0].tolist() == [0, 0, 0, 3, 3] and idx[0].tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2]       # (y 2) / 5, (x 3) / 9
    assert sr.tile_index((5, 9), (1, 1)).max() == 0
    idx = sr.tile_index((30, 60), (6, 12))
    assert np.bincount(idx).tolist() == [25] * 72
    a = hr.row_weights(5, 'solid_angle')
    area = sr.tile_area((5, 9), (2, 3), a)
    assert area.tolist() == [3 * int(a[:3].sum())] * 3 + [3 * int(a[3:].sum())] * 3 and area.sum() == 9 * a.sum()
    sp = streaming.StreamPlanner(grid_hw=(5, 9), src_hw=(2, 4), tiles=(2, 3), device='cpu')
    assert np.array_equal(sp.area, area) and sp.area.dtype == np.int64
    sp = streaming.StreamPlanner(grid_hw=(30, 60), src_hw=(2, 4), tiles=(6, 12), weights='uniform', device='cpu')
    assert sp.area.tolist() == [25 * 1024] * 72


def test_restatement_identities():
    c = sr.case('s7x14_g30x60')
    S, P = c['ins'].shape
    hs, ws = c['src']
    # a one-hot map gives its camera's footprint
    for j in (0, 37, S - 1):
        sal = np.zeros((1, hs, ws), np.float32)
        sal.reshape(-1)[j] = 2.5
        out, tot = sr.expect64(sal, c['a_src'], c['ins'])
        assert np.array_equal(out[0], c['ins'][j].astype(np.float64)) and tot[0] == 2.5 * c['a_src'][j // ws]
        out32, tot32 = sr.expect32(sal, c['a_src'], c['ins'])
        assert np.array_equal(out32[0], c['ins'][j].astype(np.float32)) and tot32.dtype == np.float32
    # linear in the masses: the expectation of a sum is the total-weighted mean of the expectations
    A, B = sr.random_maps(11, 2, c['src']), sr.random_maps(12, 2, c['src'])
    (oa, ta), (ob, tb), (oc, tc) = (sr.expect64(m, c['a_src'], c['ins']) for m in (A, B, A + B))
    # ... up to the one float32 rounding of every entry of A + B
    assert np.max(np.abs(oc * tc[:, None] - (oa * ta[:, None] + ob * tb[:, None])) / tc[:, None]) <= 2.0 ** -24
    # what is not positive and finite has no mass
    bad = A.copy()
    bad[0, 0, :4] = [np.nan, np.inf, -1.0, 0.0]
    clean = bad.copy()
    clean[0, 0, :4] = 0.0
    for x, y in zip(sr.expect32(bad, c['a_src'], c['ins']), sr.expect32(clean, c['a_src'], c['ins'])):
        assert np.array_equal(x, y)
    zero = sr.expect32(np.zeros((1, hs, ws), np.float32), c['a_src'], c['ins'])
    assert not zero[0].any() and zero[1][0] == 0.0
    # float32 in its order stays within the bound derived for it: S additions, one product and one quotient
    e = (S + 2) * 2.0 ** -24
    o32, o64 = sr.expect32(A, c['a_src'], c['ins'])[0], oa
    assert np.all(o64 * (1 - e) <= o32) and np.all(o32 <= o64 * (1 + e))
    # a tile is needed by whoever sees any of its pixels: vis >= the largest coverage in the tile
    tinc = sr.tile_or(c['ins'], c['grid'], c['tiles'])
    vis = sr.expect64(A, c['a_src'], tinc)[0]
    idx = sr.tile_index(c['grid'], c['tiles'])
    for t in range(tinc.shape[1]):
        assert np.all(vis[:, t] >= oa[:, idx == t].max(axis=1))
    assert np.all(vis <= 1.0) and np.all(oa <= 1.0)


@pytest.mark.parametrize('view', [sr.SQ100, ((9, 16), 75.0)])
def test_coverage_sums_to_the_window_solid_angle(view):
    """sum_i a_i cov[i] is the expected area of the window: every camera's footprint has the window's solid angle, within the
    weight of the pixels that its edge cuts (K17's bound for one footprint, here for the worst of the cameras)."""
    src, (h, w) = (4, 8), (60, 120)
    cams = sr.cameras(src)
    ins = hr.masks(cams.astype(np.float64), h, w, view)
    a = hr.row_weights(h, 'solid_angle')
    px_area = (math.pi / h) * (2.0 * math.pi / w) / 1024.0
    omega = sr.window_solid_angle(view)
    slack = 0.0
    for m in ins:
        nb = np.roll(m, 1, 1) & np.roll(m, -1, 1) & np.vstack([m[:1], m[:-1]]) & np.vstack([m[1:], m[-1:]])
        slack = max(slack, 2.0 * float((a[:, None] * (m & ~nb)).sum()) * px_area + m.sum() * px_area * 0.5)
    cov = sr.expect64(sr.random_maps(13, 3, src), hr.row_weights(src[0], 'solid_angle'), ins.reshape(len(cams), -1))[0]
    got = (cov.reshape(3, h, w) * a[None, :, None]).sum(axis=(1, 2)) * px_area
    print('window %r: solid angle %.4f, expected coverage area %s, slack %.4f' % (view, omega, got, slack))
    assert np.all(np.abs(got - omega) <= slack) and np.all(np.abs(got - omega) <= 0.1 * omega)


def test_qarea_restatement():
    c = sr.case('s4x8_g12x24')
    R = hr.random_cameras(31, 5)
    off = np.array([0, 2, 2, 5], np.int32)
    masks = hr.masks(R.astype(np.float64), 12, 24, c['view'])
    levels = (np.arange(3 * 12).reshape(3, 12) * 7) % 5
    q = sr.qarea(masks, off, c['grid'], c['tiles'], c['a_grid'], levels, 3)
    own = hr.agreement(R, c['view'], R, np.arange(6), 12, 24, c['view'], c['a_grid'])[1]
    assert q.shape == (5, 3) and np.array_equal(q.sum(axis=1), own)
    q5 = sr.qarea(masks, off, c['grid'], c['tiles'], c['a_grid'], levels, 5)
    assert np.array_equal(q5[:, :2], q[:, :2]) and np.array_equal(q5[:, 2:].sum(axis=1), q[:, 2])       # a level >= L counts as L - 1


# ----------------------------------------------------------------------------- segments
def test_segment_offsets():
    assert streaming.segment_offsets(24, 8.0).tolist() == [0, 8, 16, 24]
    assert streaming.segment_offsets(26, 8.0).tolist() == [0, 8, 16, 24, 26]                  # the last one is short
    assert streaming.segment_offsets(26, 8.0, seconds=2.0).tolist() == [0, 16, 26]
    assert streaming.segment_offsets(26, 8.0, cuts=[5, 21]).tolist() == [0, 5, 13, 21, 26]    # never across a cut
    assert streaming.segment_offsets(26, 8.0, cuts=[8]).tolist() == [0, 8, 16, 24, 26]
    assert streaming.segment_offsets(3, 30.0).tolist() == [0, 3]
    assert streaming.segment_offsets(5, 0.4).tolist() == [0, 1, 2, 3, 4, 5]                   # at least a frame
    assert streaming.segment_offsets(24, 8.0).dtype == np.int64
    for bad in ((0, 8.0, 1.0), (5, 0.0, 1.0), (5, 8.0, 0.0), (5, float('nan'), 1.0)):
        with pytest.raises(ValueError):
            streaming.segment_offsets(*bad)
    with pytest.raises(ValueError):
        streaming.segment_offsets(10, 8.0, cuts=[12])


def test_demand_is_the_maximum_over_a_segment():
    vis = torch.tensor([[0.1, 0.0], [0.3, 0.0], [0.2, 0.5], [0.0, 0.4], [0.9, 0.0]])
    d = streaming.StreamPlanner.demand(vis, [0, 2, 4, 5])
    assert torch.equal(d, torch.tensor([[0.3, 0.0], [0.2, 0.5], [0.9, 0.0]]))
    for seg in ([0, 2, 4], [1, 5], [0, 2, 2, 5], [0]):
        with pytest.raises(ValueError):
            streaming.StreamPlanner.demand(vis, seg)


# ----------------------------------------------------------------------------- the allocation
RATES = [1.0e6, 4.0e6, 1.6e7]


def _cost(levels, area, rates, seconds=1.0):
    area = np.asarray(area, np.float64)
    return (np.asarray(rates)[np.asarray(levels)] * area[None, :] / area.sum() * seconds).sum(axis=1)


def test_allocate_respects_the_budget_and_the_demand():
    from cp_360_weakly_supervised_saliency_amd.utils import hashrng
    area = np.array([3, 3, 3, 5, 5, 5, 4, 4], np.int64) * 1024         # a sum of 2^15: every cost is exact in float64
    demand = np.abs(hashrng.normal(41, (6, 8), dtype=np.float64))
    demand[2, 3] = 0.0
    demand[4] = 0.0
    for budget in (1.0e6, 2.5e6, 4.0e6, 9.0e6, 1.6e7, 1.0e9):
        lv = streaming.allocate(demand, area, RATES, budget)
        assert lv.shape == (6, 8) and lv.dtype == np.int64 and lv.min() >= 0 and lv.max() <= 2
        assert np.all(_cost(lv, area, RATES) <= budget * (1 + 1e-12)), budget
        assert lv[2, 3] == 0 and not lv[4].any()                       # demand 0 stays at 0
        assert np.array_equal(lv, streaming.allocate(demand, area, RATES, budget))            # deterministic
        assert np.array_equal(lv, streaming.allocate(torch.from_numpy(demand), area, RATES, budget))
        assert np.allclose(streaming.plan_bits(lv, area, RATES), _cost(lv, area, RATES), rtol=1e-12)
        for g in range(6):                                             # more demand on no more area: no lower level
            for a in range(8):
                for b in range(8):
                    if demand[g, a] > demand[g, b] and area[a] <= area[b]:
                        assert lv[g, a] >= lv[g, b], (budget, g, a, b)
    top = streaming.allocate(demand, area, RATES, 1.6e7)               # everything at the top fits: the top wherever demand is positive
    assert np.array_equal(top, np.where(demand > 0, 2, 0))
    assert not streaming.allocate(demand, area, RATES, 1.0e6).any()    # exactly all-at-0
    # seconds scale the cost
    assert np.array_equal(streaming.allocate(demand, area, RATES, 5.0e6, seconds=2.0), streaming.allocate(demand, area, RATES, 2.5e6))


def test_allocate_ties_and_refusals():
    area = np.full(4, 100, np.int64)
    lv = streaming.allocate(np.full((1, 4), 0.5), area, RATES, 1.0e6 + 2 * 0.75e6 + 1.0)      # room for two upgrades to level 1
    assert lv.tolist() == [[1, 1, 0, 0]]                               # ties go to the lowest tile
    lv = streaming.allocate(np.array([[0.5, 0.5, 0.5, 0.6]]), area, RATES, 1.0e6 + 2 * 0.75e6 + 1.0)
    assert lv.tolist() == [[1, 0, 0, 1]]
    # log utility: the slope from level 0 (ln 4 / 3e6) is 4 times the one from level 1 (ln 4 / 12e6): a tile with 5 times the
    # demand goes to the top before the others leave level 0
    lv = streaming.allocate(np.array([[5.0, 1.0, 1.0, 1.0]]), area, RATES, 1.0e6 + 0.75e6 + 3.0e6 + 1.0)
    assert lv.tolist() == [[2, 0, 0, 0]]
    with pytest.raises(ValueError, match='budget'):
        streaming.allocate(np.ones((1, 4)), area, RATES, 0.99e6)       # below all-at-0
    with pytest.raises(ValueError, match='concave'):
        streaming.allocate(np.ones((1, 4)), area, RATES, 1e7, utility=[0.0, 1.0, 6.0])       # slopes 1 / 3e6 < 5 / 12e6
    for rates in ([4e6, 1e6], [0.0, 1e6], [1e6, 1e6], [], [float('nan'), 1.0], list(range(1, 10))):
        with pytest.raises(ValueError):
            streaming.allocate(np.ones((1, 4)), area, rates, 1e9)
    with pytest.raises(ValueError):
        streaming.allocate(np.ones((1, 4)), area, RATES, 1e9, utility=[0.0, 1.0])
    with pytest.raises(ValueError):
        streaming.allocate(np.ones((1, 4)), area, RATES, 1e9, utility=[2.0, 1.0, 0.0])
    with pytest.raises(ValueError):
        streaming.allocate(np.ones((1, 3)), area, RATES, 1e9)
    with pytest.raises(ValueError):
        streaming.allocate(-np.ones((1, 4)), area, RATES, 1e9)
    one = streaming.allocate(np.ones((2, 4)), area, [2.0e6], 2.0e6)    # a ladder of one level
    assert one.shape == (2, 4) and not one.any()


def test_uniform():
    area = np.array([1, 1, 2], np.int64)                               # a sum of 4: every cost is exact
    assert streaming.uniform(area, RATES, 1.0e6) == 0 and streaming.uniform(area, RATES, 3.99e6) == 0
    assert streaming.uniform(area, RATES, 4.0e6) == 1 and streaming.uniform(area, RATES, 1e9) == 2
    assert streaming.uniform(area, RATES, 8.0e6, seconds=2.0) == 1
    with pytest.raises(ValueError):
        streaming.uniform(area, RATES, 0.5e6)


# ----------------------------------------------------------------------------- library
def test_library_exports_the_symbols():
    hdr = open(os.path.join(REPO, 'include', 'cp360.h')).read()
    declared = set(re.findall(r'\b(cp360_[a-z0-9_]+)\s*\(', hdr))
    L = _lib.lib()
    for name in K24:
        assert name in declared and name in _lib.PUBLIC_SYMBOLS and hasattr(L, name)
    hv = int(re.search(r'#define\s+CP360_VERSION\s+(\d+)', hdr).group(1))
    assert L.cp360_version() == hv == _lib.ABI_VERSION == 306


def _bad(fn, ok, **kw):
    args = list(ok)
    for k, v in kw.items():
        args[int(k[1:])] = v
    return fn(*args)


def test_status_codes_without_gpu():
    """Argument validation happens before any launch: the dummy pointers are never used."""
    L = _lib.lib()
    one, big, PI = C.c_void_p(16), 1 << 40, math.pi
    inc = lambda *a: L.cp360_view_incidence(*a, None)
    tinc = lambda *a: L.cp360_tile_incidence(*a, None)
    exp = lambda *a: L.cp360_view_expect(*a, None)
    qual = lambda *a: L.cp360_view_quality(*a, None)
    ok_i = [one, 8, 8, 16, 1.7, 1.0, one, one, big]                    # cams S h w hfov aspect inc work bytes
    ok_t = [one, 8, 8, 16, 2, 4, one]                                  # inc S h w rows cols tinc
    ok_e = [one, 3, 2, 4, one, one, 128, one, one]                     # sal F hs ws weights bits P out total
    ok_q = [one, one, 5, 2, 8, 16, 1.7, 1.0, one, one, 2, 4, 3, one, one, big]       # R off N F h w hfov aspect a levels rows cols L qarea work bytes
    for k in (0, 6, 7):
        assert _bad(inc, ok_i, **{'a%d' % k: None}) == NULL, k
    for k in (0, 6):
        assert _bad(tinc, ok_t, **{'a%d' % k: None}) == NULL, k
    for k in (0, 4, 5, 7, 8):
        assert _bad(exp, ok_e, **{'a%d' % k: None}) == NULL, k
    for k in (0, 1, 8, 9, 13, 14):
        assert _bad(qual, ok_q, **{'a%d' % k: None}) == NULL, k
    # shapes
    for S, h, w in ((0, 8, 16), (8, 0, 16), (8, 8, 0), (-1, 8, 16), (8, -8, 16)):
        assert _bad(inc, ok_i, a1=S, a2=h, a3=w) == BAD_SHAPE and _bad(tinc, ok_t, a1=S, a2=h, a3=w) == BAD_SHAPE
    for rows, cols in ((0, 4), (2, 0), (9, 4), (2, 17), (-1, 4)):
        assert _bad(tinc, ok_t, a4=rows, a5=cols) == BAD_SHAPE and _bad(qual, ok_q, a10=rows, a11=cols) == BAD_SHAPE
    for fov in (0.0, -0.5, PI, 4.0, float('nan'), float('inf')):
        assert _bad(inc, ok_i, a4=fov) == BAD_SHAPE and _bad(qual, ok_q, a6=fov) == BAD_SHAPE
    for asp in (0.0, -1.0, float('nan'), float('inf'), 1e39):
        assert _bad(inc, ok_i, a5=asp) == BAD_SHAPE and _bad(qual, ok_q, a7=asp) == BAD_SHAPE
    for F, hs, ws, P in ((-1, 2, 4, 128), (3, 0, 4, 128), (3, 2, 0, 128), (3, 2, 4, 0)):
        assert _bad(exp, ok_e, a1=F, a2=hs, a3=ws, a6=P) == BAD_SHAPE
    for L_ in (0, 9, -1):
        assert _bad(qual, ok_q, a12=L_) == BAD_SHAPE
    assert _bad(qual, ok_q, a2=-1) == BAD_SHAPE and _bad(qual, ok_q, a3=-1) == BAD_SHAPE and _bad(qual, ok_q, a3=0) == BAD_SHAPE
    for h, w in ((0, 16), (8, 0)):
        assert _bad(qual, ok_q, a4=h, a5=w) == BAD_SHAPE
    # limits
    assert _bad(inc, ok_i, a1=4097) == UNSUPPORTED
    assert _bad(inc, ok_i, a2=1024, a3=2049) == UNSUPPORTED and _bad(tinc, ok_t, a2=1024, a3=2049) == UNSUPPORTED
    assert _bad(tinc, ok_t, a1=4097) == UNSUPPORTED and _bad(tinc, ok_t, a2=128, a3=128, a4=64, a5=65) == UNSUPPORTED
    assert _bad(exp, ok_e, a1=65536) == UNSUPPORTED and _bad(exp, ok_e, a2=64, a3=65) == UNSUPPORTED
    assert _bad(exp, ok_e, a6=(1 << 21) + 1) == UNSUPPORTED
    assert _bad(qual, ok_q, a3=65536) == UNSUPPORTED and _bad(qual, ok_q, a2=1 << 31) == UNSUPPORTED
    assert _bad(qual, ok_q, a4=1024, a5=2049) == UNSUPPORTED and _bad(qual, ok_q, a4=128, a5=128, a10=64, a11=65) == UNSUPPORTED
    # alignment
    for k in (0, 6):
        assert _bad(inc, ok_i, **{'a%d' % k: C.c_void_p(18)}) == ALIGN and _bad(tinc, ok_t, **{'a%d' % k: C.c_void_p(18)}) == ALIGN
    assert _bad(inc, ok_i, a7=C.c_void_p(8)) == ALIGN and _bad(qual, ok_q, a14=C.c_void_p(8)) == ALIGN
    for k in (0, 4, 5, 7, 8):
        assert _bad(exp, ok_e, **{'a%d' % k: C.c_void_p(18)}) == ALIGN, k
    for k in (0, 1, 8):
        assert _bad(qual, ok_q, **{'a%d' % k: C.c_void_p(18)}) == ALIGN, k
    assert _bad(qual, ok_q, a13=C.c_void_p(20)) == ALIGN
    # workspaces
    tables = L.cp360_fix_work_bytes(0, 8, 16)
    need = L.cp360_view_quality_work_bytes(8, 16)
    assert need % 16 == 0 and need >= tables + (8 + 16) * 4
    assert L.cp360_view_quality_work_bytes(0, 16) == 0 == L.cp360_view_quality_work_bytes(1024, 2049)
    assert _bad(inc, ok_i, a8=tables - 1) == BAD_SHAPE and _bad(qual, ok_q, a15=need - 1) == BAD_SHAPE
    # nothing to launch: no frames, no viewers
    assert _bad(exp, ok_e, a1=0) == 0 and _bad(exp, ok_e, a1=0, a0=None, a7=None, a8=None) == 0
    assert _bad(qual, ok_q, a2=0, a15=need) == 0 and _bad(qual, ok_q, a2=0, a0=None, a9=None, a13=None, a15=need) == 0
    assert _bad(qual, ok_q, a2=0, a3=0, a15=need) == 0 and _bad(qual, ok_q, a2=0, a15=need - 1) == BAD_SHAPE


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    cams = torch.zeros(8, 3, 3)
    a = torch.full((2,), 1024, dtype=torch.int32)
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.view_incidence(cams, (5, 9), (1, 1), 100.0)
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.tile_incidence(torch.zeros(8, 2, dtype=torch.int32), (5, 9), (2, 3))
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.view_expect(torch.zeros(1, 2, 4), a, torch.zeros(8, 2, dtype=torch.int32), 45)
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.view_quality(torch.zeros(4, 3, 3), torch.tensor([0, 4], dtype=torch.int32), (5, 9), ((1, 1), 100.0),
                         torch.full((5,), 1024, dtype=torch.int32), torch.zeros(1, 6, dtype=torch.uint8), (2, 3), 3)
    with pytest.raises(RuntimeError, match='GPU only'):
        streaming.StreamPlanner(grid_hw=(5, 9), src_hw=(2, 4), tiles=(2, 3), device='cpu').coverage(np.zeros((1, 2, 4), np.float32))
    for hw, tiles in (((0, 9), (1, 1)), ((1024, 2049), (1, 1)), ((5, 9), (6, 3)), ((5, 9), (2, 10)), ((5, 9), (0, 3)), ((128, 128), (64, 65))):
        with pytest.raises(ValueError):
            ops._stream_grid(hw, tiles)
        with pytest.raises(ValueError):
            streaming.StreamPlanner(grid_hw=hw, tiles=tiles)
    assert ops._stream_grid((5, 9)) == (5, 9, 1, 1) and ops._stream_grid((5, 9), (2, 3)) == (5, 9, 2, 3)
    for kw in (dict(src_hw=(0, 4)), dict(src_hw=(64, 65)), dict(hfov_deg=180.0), dict(view_hw=(0, 1)), dict(weights='flat')):
        with pytest.raises(ValueError):
            streaming.StreamPlanner(**kw)
