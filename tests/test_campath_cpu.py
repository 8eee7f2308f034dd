"""K16, the camera path by dynamic programming, without a GPU: the exports and their status codes, the host's turn-cost table
against its restatement (exactly), the table's properties, and the restatement's own claims - that its programme finds the best of
all paths, and that the planned path does what it is for on the videos of tests/campath_restate.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from cp_360_weakly_supervised_saliency_amd import _lib, ops
from cp_360_weakly_supervised_saliency_amd.utils.viewport import ViewportPilot
from tests import campath_restate as cr
from tests import viewport_restate as vr

TABLES = [((5, 9), 16.0, 45.0), ((9, 16), 16.0, 25.0), ((14, 28), 16.0, 15.0), ((32, 64), 16.0, 15.0)]
EXPORTS = ['cp360_path_table_bytes', 'cp360_path_table_host', 'cp360_path_work_bytes', 'cp360_view_path', 'cp360_view_refine']


# ----------------------------------------------------------------------------- exports
def test_exports_and_status_codes_before_any_launch():
    L = _lib.lib()
    assert L.cp360_version() == _lib.ABI_VERSION == 306
    for name in EXPORTS:
        assert name in _lib.PUBLIC_SYMBOLS and hasattr(L, name)
    half = 28 // 2 + 1
    assert L.cp360_path_table_bytes(14, 28) == 4 * (14 * 14 * half + 14 * 14)
    assert L.cp360_path_table_bytes(0, 28) == 0 and L.cp360_path_table_bytes(129, 128) == 0
    tabs = _lib.lib().cp360_stab_work_bytes(0, 14, 28)
    assert L.cp360_path_work_bytes(24, 14, 28) == tabs + 24 * 14 * 28 * 2
    assert L.cp360_path_work_bytes(0, 14, 28) == 0 and L.cp360_path_work_bytes(65536, 14, 28) == 0
    assert L.cp360_path_work_bytes(1, 128, 129) == 0
    out = np.empty(L.cp360_path_table_bytes(5, 9) // 4, np.int32)
    po = out.ctypes.data_as(C.c_void_p)
    assert L.cp360_path_table_host(5, 9, 16.0, 0.5, None) == -5
    assert L.cp360_path_table_host(0, 9, 16.0, 0.5, po) == -1
    assert L.cp360_path_table_host(5, 9, -1.0, 0.5, po) == -1
    assert L.cp360_path_table_host(5, 9, 4097.0, 0.5, po) == -1
    assert L.cp360_path_table_host(5, 9, float('nan'), 0.5, po) == -1
    assert L.cp360_path_table_host(5, 9, 16.0, 0.0, po) == -1
    assert L.cp360_path_table_host(5, 9, 16.0, 3.2, po) == -1
    assert L.cp360_path_table_host(5, 9, 16.0, float('inf'), po) == -1
    assert L.cp360_path_table_host(129, 128, 16.0, 0.5, po) == -8
    assert L.cp360_path_table_host(5, 9, 16.0, 0.5, po) == 0
    d, odd = C.c_void_p(16), C.c_void_p(24)
    big = 1 << 40
    path = lambda **kw: L.cp360_view_path(*[kw.get(k, v) for k, v in (
        ('smooth', d), ('gain', d), ('F', 8), ('hm', 14), ('wm', 28), ('table', d), ('starts', d), ('S', 1), ('idx', d), ('dirs', d),
        ('score', d), ('work', d), ('bytes', big), ('stream', None))])
    for name in ('smooth', 'gain', 'table', 'starts', 'idx', 'dirs', 'score', 'work'):
        assert path(**{name: None}) == -5, name
    assert path(F=0) == -1 and path(hm=0) == -1 and path(wm=-3) == -1
    assert path(S=0) == -1 and path(S=9) == -1
    assert path(hm=129, wm=128) == -8 and path(F=65536, S=2) == -8
    assert path(work=odd) == -6
    assert path(bytes=L.cp360_path_work_bytes(8, 14, 28) - 1) == -1
    fine = lambda **kw: L.cp360_view_refine(*[kw.get(k, v) for k, v in (
        ('maps', d), ('idx', d), ('F', 8), ('hm', 14), ('wm', 28), ('sigma', 0.26), ('dirs', d), ('work', d), ('bytes', big),
        ('stream', None))])
    for name in ('maps', 'idx', 'dirs', 'work'):
        assert fine(**{name: None}) == -5, name
    assert fine(F=0) == -1 and fine(sigma=0.0) == -1 and fine(sigma=float('nan')) == -1
    assert fine(hm=129, wm=128) == -8 and fine(F=65536) == -8
    assert fine(work=odd) == -6 and fine(bytes=tabs - 1) == -1


def test_wrappers_refuse_bad_arguments():
    with pytest.raises(ValueError):
        ViewportPilot(planner='greedy')
    with pytest.raises(ValueError):
        ViewportPilot(planner='viterbi', turn_cost=-1.0)
    with pytest.raises(ValueError):
        ViewportPilot(planner='viterbi', plan_step_deg=0.0)
    assert ViewportPilot().planner == 'peak'
    maps = torch.zeros((4, 14, 28))
    with pytest.raises(ValueError):                                   # 180 / 14 = 12.9 degrees between two rows
        ViewportPilot(planner='viterbi', plan_step_deg=12.0).plan(maps)
    with pytest.raises(ValueError):
        ViewportPilot(planner='viterbi').plan(maps[0])
    with pytest.raises(ValueError):
        ViewportPilot(planner='viterbi').plan(maps, cuts=[4])
    with pytest.raises(ValueError):
        ops.path_table_host(14, 28, 16.0, 12.0)
    with pytest.raises(ValueError):
        ops.path_table_host(14, 28, 5000.0, 15.0)
    with pytest.raises(ValueError):
        ops.path_table_host(14, 28, 16.0, 181.0)
    with pytest.raises(ValueError):
        ops.path_table_host(129, 128, 16.0, 15.0)
    with pytest.raises(RuntimeError):
        ops.sphere_path(maps, torch.ones(4))
    with pytest.raises(RuntimeError):
        ops.sphere_refine(maps, torch.zeros(4, dtype=torch.int32))


# ----------------------------------------------------------------------------- the table
@pytest.mark.parametrize('hw,turn_cost,step_deg', TABLES)
def test_table_equals_the_restatement(hw, turn_cost, step_deg):
    hm, wm = hw
    cost, span, (round_margin, limit_margin) = cr.path_table(hm, wm, turn_cost, step_deg)
    print('%d x %d: nearest rounding boundary %.3g, nearest angle to the limit %.3g degrees' % (hm, wm, round_margin, limit_margin))
    assert round_margin > 1e-6 and limit_margin > 1e-6                # no entry hangs on the last bits: equality is not luck
    table = ops.path_table_host(hm, wm, turn_cost, step_deg)
    assert table.dtype == np.int32 and table.shape == (hm * hm * (wm // 2 + 1) + hm * hm,)
    got_cost, got_span = ops.path_table_split(table, hm, wm)
    assert np.array_equal(got_cost, cost) and np.array_equal(got_span, span)


@pytest.mark.parametrize('hw,turn_cost,step_deg', TABLES + [((6, 7), 0.0, 180.0), ((3, 4), 4096.0, 90.0)])
def test_table_properties(hw, turn_cost, step_deg):
    hm, wm = hw
    cost, span = ops.path_table_split(ops.path_table_host(hm, wm, turn_cost, step_deg), hm, wm)
    assert np.array_equal(cost, cost.transpose(1, 0, 2)) and np.array_equal(span, span.T)
    assert np.all(cost[np.arange(hm), np.arange(hm), 0] == 0)
    d = np.arange(wm // 2 + 1)
    assert np.array_equal(cost >= 0, d[None, None, :] <= span[:, :, None])   # one interval from 0, and span is its end
    assert np.all(cost[cost < 0] == -1) and cost.max() <= 4096 * 180
    assert np.all(np.diff(np.where(cost >= 0, cost, 1 << 30), axis=2) >= 0)  # the cost grows with the column difference
    if step_deg == 180.0:
        assert np.all(span == wm // 2)
    if turn_cost == 0.0:
        assert np.all(cost[cost >= 0] == 0)
    # the angle of the restatement's geometry: the neighbouring rows of one column are 180 / hm degrees apart
    if step_deg >= 180.0 / hm and hm > 1:
        assert cost[0, 1, 0] == np.rint(turn_cost * 180.0 / hm)


# ----------------------------------------------------------------------------- the restatement's own claims
def test_programme_finds_the_best_of_all_paths():
    hm, wm, F = 3, 4, 4
    rng = np.random.RandomState(16)
    for turn_cost, step_deg in ((16.0, 95.0), (3.0, 61.0)):
        q = rng.randint(0, 4097, size=(F, hm, wm)).astype(np.int64)
        want, count = cr.brute_force_score(q, hm, wm, turn_cost, step_deg)
        assert count == 20736
        idx, score, acc = cr.programme(q, hm, wm, turn_cost, step_deg)
        assert score == want
        # ... and the path the trace returns has that score and only allowed moves
        cost, span, _ = cr.path_table(hm, wm, turn_cost, step_deg)
        total = int(q.reshape(F, -1)[np.arange(F), idx].sum())
        for t in range(1, F):
            (ri, ci), (rj, cj) = divmod(int(idx[t - 1]), wm), divmod(int(idx[t]), wm)
            d = min(abs(ci - cj), wm - abs(ci - cj))
            assert cost[ri, rj, d] >= 0
            total -= int(cost[ri, rj, d])
        assert total == score


def test_votes():
    s = np.array([[[0.5, -1.0, np.nan, np.inf], [2.0, 1e30, 0.00012, 0.00037]]], np.float32)
    q = cr.votes(s, np.array([4096.0], np.float32))[0]
    assert q.tolist() == [[2048, 0, 0, 0], [4096, 4096, 0, 2]]        # 0.49 rounds down, 1.52 up; 1e30 is finite: clamped
    assert cr.votes(s, np.array([np.nan], np.float32)).max() == 0
    assert cr.votes(np.array([[[0.5, 1.5, 2.5]]], np.float32), np.array([1.0], np.float32))[0].tolist() == [[0, 2, 2]]


def test_two_people_talking():
    """The peaks hop between the two blobs and the path filter averages the hops: the 'peak' chain ends between them.  The planned
    chain stays with one of them.  Measured: the 'peak' chain 50.9 degrees from the nearer blob at the end (51 - 54 over the
    second half), the planned chain 1.1 - 1.3 degrees from one blob throughout at 14 x 28 and 0.6 at 32 x 64."""
    hm, wm = 14, 28
    maps, blobs = cr.two_blob_video(hm, wm)
    F = maps.shape[0]
    raw, chain = cr.peak_chain(maps)
    hops = cr.angles_deg(raw[1:], raw[:-1])
    assert np.all(hops > 90.0)                                         # every frame's peak is the other blob
    near = np.minimum(cr.angles_deg(chain, blobs[0]), cr.angles_deg(chain, blobs[1]))
    print('peak chain, degrees from the nearer blob:', near.round(1).tolist())
    assert near[-1] >= 40.0 and near[F // 2:].min() >= 40.0
    idx, fine, planned = cr.plan_chain(maps)
    per_blob = [cr.angles_deg(planned, b).max() for b in blobs]
    print('planned chain, largest distance from each blob: %.2f, %.2f degrees' % tuple(per_blob))
    assert min(per_blob) <= cr.half_diagonal_deg(hm, wm) <= 9.1


@pytest.mark.parametrize('where', ['seam', 'pole'])
def test_a_brief_distractor(where):
    """A blob 1.6 times as high for two frames pulls the per-frame argmax away; the planned path does not leave the moving blob.
    Measured at 14 x 28: the argmax up to 172 / 120 degrees off, the path's pixel centres at most 8.6 / 7.2 degrees (half a pixel's
    diagonal is 9.1), the refined directions 3.5 / 2.9."""
    hm, wm = 14, 28
    maps, truth = cr.distractor_video(hm, wm, where)
    raw, _ = cr.peak_chain(maps)
    assert cr.angles_deg(raw, truth).max() > 100.0
    idx, fine, _ = cr.plan_chain(maps)
    off_raw, off_fine = cr.angles_deg(cr.centres(idx, hm, wm), truth), cr.angles_deg(fine, truth)
    print('%s: pixel centres at most %.2f, refined at most %.2f degrees off' % (where, off_raw.max(), off_fine.max()))
    assert off_raw.max() <= 9.1 and off_fine.max() <= 9.1
    rows, cols = idx // wm, idx % wm
    if where == 'seam':
        assert (np.abs(np.diff(cols)) > wm // 2).any()                 # from the last column to the first
        assert cols.max() == wm - 1 and cols.min() == 0
    else:
        assert rows.min() == 0 and (np.abs(np.diff(cols)) >= wm // 2 - 1).any()   # into the first row and out on the far side


def test_a_cut_frees_the_path():
    hm, wm = 14, 28
    maps, truth = cr.jump_video(hm, wm)
    idx, _, _ = cr.plan_chain(maps)
    c = cr.centres(idx, hm, wm)
    assert cr.angles_deg(c[1:], c[:-1]).max() <= 15.0                  # one take: no step beyond the limit
    idx, fine, _ = cr.plan_chain(maps, cuts=[12])
    c = cr.centres(idx, hm, wm)
    steps = cr.angles_deg(c[1:], c[:-1])
    assert steps[11] > 120.0 and np.delete(steps, 11).max() <= 15.0    # two takes: the path jumps with the blob
    assert cr.angles_deg(fine, truth).max() <= 9.1
    assert vr.angle(c[0], truth[0]) < np.deg2rad(9.1)
