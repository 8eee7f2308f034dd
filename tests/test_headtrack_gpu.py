"""GPU tests of the head-tracking ground truth (K17, csrc/headtrack.hip) against tests/headtrack_restate.py: the footprint counts
and the agreement sums within what float64 leaves float32 to decide (tests/test_headtrack_cpu.py asserts the cap on that for
every case), the identities that hold exactly because both kernels decide with one function, and the drivers end to end."""
import os

import numpy as np
import pytest
import torch

from cp_360_weakly_supervised_saliency_amd import _lib, ops
from cp_360_weakly_supervised_saliency_amd.utils import eval_sphere, fixations, headtrack, npy_io, viewport
from tests import headtrack_restate as hr
from tests import viewport_restate as vr

pytestmark = pytest.mark.gpu


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def run_case(c, work=None):
    R, off = dev(c['R']), dev(c['offsets'])
    a = ops.sphere_eval_weights(c['grid'][0], c['mode'], R.device)
    counts, n_views = ops.head_footprints(R, off, c['grid'], c['view'][0], c['view'][1], work=work)
    inter, uni = ops.head_agreement(dev(c['Rc']), c['cam_view'], R, off, c['grid'], c['view'], a, work=work)
    return counts.cpu().numpy(), n_views.cpu().numpy(), inter.cpu().numpy(), uni.cpu().numpy()


# ----------------------------------------------------------------------------- against float64
@pytest.mark.parametrize('name', sorted(hr.CASES))
def test_against_float64(name):
    check_against_float64(hr.case(name))


def check_against_float64(c):
    name = c['name']
    n_in, n_und = int(c['ins'].sum()), int(c['und'].sum())
    assert n_und <= 0.001 * n_in and int(c['cund'].sum()) <= 0.001 * int(c['cins'].sum())
    counts, n_views, inter, uni = run_case(c)
    F, N = len(c['offsets']) - 1, len(c['R'])
    assert counts.shape == (F,) + c['grid'] and counts.dtype == np.int32 and inter.shape == (N,) == uni.shape and inter.dtype == np.int64
    lo, hi = hr.count_bounds(c)
    print('%s: %d inside pairs, %d undecided; counts differ from the decided ones in %d pixels'
          % (name, n_in, n_und, int((counts != lo).sum())))
    assert np.all(lo <= counts) and np.all(counts <= hi)
    finite = np.array([bool(np.all(np.isfinite(r))) for r in c['R']], bool)
    assert n_views.tolist() == [int(finite[c['offsets'][f]:c['offsets'][f + 1]].sum()) for f in range(F)]
    b = hr.agreement_bounds(c)
    assert np.all(b[0] <= inter) and np.all(inter <= b[1]) and np.all(b[2] <= uni) and np.all(uni <= b[3])
    if name == 'uniform_12x24':
        assert np.all(inter % 1024 == 0) and np.all(uni % 1024 == 0)
    if name == 'gaps_30x60':                                           # the NaN and the inf viewer, and the inf camera of frame 3
        assert inter[3] == 0 == inter[25] and uni[3] > 0 and uni[25] > 0 and np.all(inter[50:] == 0) and np.all(uni[50:] > 0) and counts[1].sum() == 0 == counts[4].sum()


# ----------------------------------------------------------------------------- exact identities
def self_agreement(R, view, grid, a, work=None):
    """Every camera against itself with the same view, one per frame: (inter, uni)."""
    one = torch.arange(R.shape[0] + 1, dtype=torch.int32, device=R.device)
    return ops.head_agreement(R, view, R, one, grid, view, a, work=work)


@pytest.mark.parametrize('name', ['chunks_12x24', 'gaps_30x60', 'uniform_12x24', 'one_frame_5x9'])
def test_identities(name):
    check_identities(hr.case(name))


def check_identities(c):
    grid, view = c['grid'], c['view']
    R, off = dev(c['R']), dev(c['offsets'])
    a = ops.sphere_eval_weights(grid[0], c['mode'], R.device)
    counts, _ = ops.head_footprints(R, off, grid, view[0], view[1])
    area, area_u = self_agreement(R, view, grid, a)
    assert torch.equal(area, area_u)                                   # a viewer equal to the camera
    mass = (counts.to(torch.int64) * a.to(torch.int64)[None, :, None]).sum(dim=(1, 2)).cpu().numpy()
    area_np = area.cpu().numpy()
    for f in range(len(c['offsets']) - 1):                             # sum a_y counts = the sum of the viewers' own areas
        assert int(mass[f]) == int(area_np[c['offsets'][f]:c['offsets'][f + 1]].sum()), f
    # the view behind, 90 degrees each: nothing shared, the union is both areas
    sq = ((1, 1), 90.0)
    flip = dev((c['R'].astype(np.float64) * np.array([-1.0, 1.0, -1.0])).astype(np.float32))
    one = torch.arange(R.shape[0] + 1, dtype=torch.int32, device=R.device)
    inter, uni = ops.head_agreement(flip, sq, R, one, grid, sq, a)
    assert int(inter.abs().sum()) == 0
    assert torch.equal(uni, self_agreement(R, sq, grid, a)[0] + self_agreement(flip, sq, grid, a)[0])
    # 'uniform' weights: uni / 1024 is the number of pixels of the union, counted by the footprints of the two cameras as one frame
    u1 = ops.sphere_eval_weights(grid[0], 'uniform', R.device)
    Rc = dev(hr.random_cameras(900, R.shape[0]))
    _, uni = ops.head_agreement(Rc, view, R, one, grid, view, u1)
    two = torch.stack([Rc, R], dim=1).reshape(-1, 3, 3).contiguous()
    pair_counts, _ = ops.head_footprints(two, 2 * one, grid, view[0], view[1])
    assert torch.equal(uni, 1024 * (pair_counts > 0).sum(dim=(1, 2)))


def test_a_frame_does_not_depend_on_the_batch():
    c = hr.case('chunks_12x24')
    first = run_case(c)
    again = run_case(c)
    for x, y in zip(first, again):
        assert np.array_equal(x, y)
    k0, k1 = int(c['offsets'][3]), int(c['offsets'][4])                # the frame with chunk + 1 viewers, alone
    R, off = dev(c['R'][k0:k1]), dev(np.array([0, k1 - k0], np.int32))
    a = ops.sphere_eval_weights(c['grid'][0], c['mode'], R.device)
    counts, n_views = ops.head_footprints(R, off, c['grid'], c['view'][0], c['view'][1])
    inter, uni = ops.head_agreement(dev(c['Rc'][3:4]), c['cam_view'], R, off, c['grid'], c['view'], a)
    assert np.array_equal(counts.cpu().numpy()[0], first[0][3]) and int(n_views[0]) == int(first[1][3])
    assert np.array_equal(inter.cpu().numpy(), first[2][k0:k1]) and np.array_equal(uni.cpu().numpy(), first[3][k0:k1])
    # ... and fifth in a batch of five
    per = [2, 1, 0, 3, k1 - k0]
    pad = hr.random_cameras(901, sum(per[:4]))
    R5, off5 = dev(np.concatenate([pad, c['R'][k0:k1]])), dev(np.concatenate([[0], np.cumsum(per)]).astype(np.int32))
    Rc5 = dev(np.concatenate([hr.random_cameras(902, 4), c['Rc'][3:4]]))
    counts5, n5 = ops.head_footprints(R5, off5, c['grid'], c['view'][0], c['view'][1])
    inter5, uni5 = ops.head_agreement(Rc5, c['cam_view'], R5, off5, c['grid'], c['view'], a)
    assert torch.equal(counts5[4], counts[0]) and int(n5[4]) == int(n_views[0])
    assert torch.equal(inter5[6:], inter) and torch.equal(uni5[6:], uni)


# ----------------------------------------------------------------------------- streams and workspaces
def test_stream_and_workspace():
    c = hr.case('gaps_30x60')
    want = run_case(c)
    work = ops.head_work(120, 240, torch.device('cuda', torch.cuda.current_device()))      # larger than the case needs, and reused
    ptr0 = work.data_ptr()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = run_case(c, work=work)
        again = run_case(hr.case('chunks_12x24'), work=work)
    torch.cuda.current_stream().wait_stream(s)
    for x, y in zip(want, got):
        assert np.array_equal(x, y)
    for x, y in zip(run_case(hr.case('chunks_12x24')), again):
        assert np.array_equal(x, y)
    assert ops.head_work(30, 60, work.device, work).data_ptr() == ptr0 and ops.head_work(240, 480, work.device, work).data_ptr() != ptr0
    # a workspace that is too small is refused before any launch
    L = _lib.lib()
    R, off = dev(c['R']), dev(c['offsets'])
    counts = torch.full((5, 30, 60), -7, dtype=torch.int32, device='cuda')
    n_views = torch.zeros(5, dtype=torch.int32, device='cuda')
    inter = torch.full((70,), -7, dtype=torch.int64, device='cuda')
    need = L.cp360_fix_work_bytes(0, 30, 60)
    a = ops.sphere_eval_weights(30, 'solid_angle', R.device)
    assert L.cp360_head_footprints(_lib.ptr(R), _lib.ptr(off), 70, 5, 30, 60, 1.7, 1.0, _lib.ptr(counts), _lib.ptr(n_views),
                                   _lib.ptr(work), need - 1, _lib.stream()) == -1
    assert L.cp360_head_agreement(_lib.ptr(dev(c['Rc'])), 1.7, 1.0, _lib.ptr(R), _lib.ptr(off), 70, 5, 30, 60, 1.7, 1.0, _lib.ptr(a),
                                  _lib.ptr(inter), _lib.ptr(inter), _lib.ptr(work), need - 1, _lib.stream()) == -1
    torch.cuda.synchronize()
    assert int((counts != -7).sum()) == 0 and int((inter != -7).sum()) == 0


# ----------------------------------------------------------------------------- end to end
def test_pilot_against_viewers_end_to_end(tmp_path):
    """A target that moves 3 degrees a frame; the pilot follows its saliency blob, twelve viewers follow it with fixed offsets of a
    few degrees.  The pilot's path agrees with the viewers better than a camera that never moves - comparisons only."""
    F, hm, wm, fps = 24, 14, 28, 30.0
    lon = np.deg2rad(-40.0 + 3.0 * np.arange(F))
    lat = np.deg2rad(10.0 + 0.5 * np.arange(F))
    target = np.stack([np.cos(lat) * np.cos(lon), np.sin(lat), np.cos(lat) * np.sin(lon)], -1)
    maps = np.stack([vr.vmf_blob(t, hm, wm, 10.0) for t in target]).astype(np.float32)
    tf = (np.arange(F) + 0.5) / fps
    d = np.deg2rad(np.array([[-6, 2], [5, -3], [0, 4], [3, 3], [-4, -4], [6, 0], [-2, 5], [1, -5], [4, 2], [-5, 1], [2, -2], [0, 0]], float))
    tracks = [(tf, lon + dx, lat + dy, np.full(F, 0.05 * k)) for k, (dx, dy) in enumerate(d)]
    R, off, viewer = headtrack.head_cameras(tracks, fps, F)
    assert off.tolist() == (12 * np.arange(F + 1)).tolist() and viewer.tolist() == list(range(12)) * F
    pilot = viewport.ViewportPilot(hw=(36, 64), hfov_deg=90.0, sigma_deg=15.0, alpha=0.5)
    head = headtrack.HeadMaps()
    R_cam = pilot.path(maps)
    res = pilot.agreement(R_cam, R, off, head=head)
    fixed = pilot.agreement(np.broadcast_to(np.eye(3, dtype=np.float32), (F, 3, 3)), R, off, head=head)
    assert res.iou.shape == (12 * F,) and res.frame_iou.shape == (F,) and res.iou.dtype == torch.float64
    assert torch.equal(res.iou, res.inter.double() / res.union.double()) and bool(res.finite.all())
    assert torch.allclose(res.frame_iou, res.iou.reshape(F, 12).mean(dim=1), rtol=0, atol=1e-12)
    m, m0 = head.means(res), head.means(fixed)
    print('pilot %s; fixed camera %s' % (m, m0))
    assert m['frames'] == F and m['pairs'] == 12 * F
    assert m['iou'] > m0['iou'] and m['centre_angle_deg'] < m0['centre_angle_deg']
    want = np.degrees([vr.angle(np.eye(3)[:, 0], R[k, :, 0]) for k in range(12 * F)])
    assert np.max(np.abs(fixed.centre_angle_deg.cpu().numpy() - want)) <= 1e-9
    # a viewer that is not finite, and a frame without viewers
    R2 = R.copy()
    R2[:12, 0, 0] = np.nan
    R2[12] = np.inf
    r2 = head.agreement(R_cam, pilot.hw, pilot.hfov_deg, R2, off)
    assert bool(torch.isnan(r2.frame_iou[0])) and not bool(torch.isnan(r2.frame_iou[1:]).any())
    assert torch.allclose(r2.frame_iou[1], res.iou[13:24].mean(), rtol=0, atol=1e-12) and head.means(r2)['frames'] == F - 1
    # the ground-truth map: the share of the viewers, into the evaluation and onto disk
    cov = head.coverage(R, off)
    counts, n_views = head.footprints(R, off)
    assert cov.dtype == torch.float32 and float(cov.max()) == 1.0 and float(cov.min()) == 0.0 and n_views.tolist() == [12] * F
    assert np.array_equal(cov.cpu().numpy(), counts.cpu().numpy().astype(np.float32) / np.float32(12.0))     # one float32 division
    assert float(head.coverage(R2, off)[0].max()) == 0.0
    ev = eval_sphere.SphereEval()
    assert float((ev.evaluate(cov, cov).cc - 1.0).abs().max()) <= 1e-9
    fixations.save_gt(str(tmp_path / 'gt'), 'vid', cov)
    for k in range(F):
        path = npy_io.saliency_path(str(tmp_path / 'pred'), 'vid', k)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        np.save(path, cov[k].cpu().numpy())
    scores = eval_sphere.evaluate_video_dir(str(tmp_path / 'pred'), str(tmp_path / 'gt'), 'vid', ev)
    assert len(scores) == F and float((scores.cc - 1.0).abs().max()) <= 1e-9


def test_no_viewers_at_all():
    c = hr.case('empty_5x9')
    counts, n_views, inter, uni = run_case(c)
    assert counts.shape == (3, 5, 9) and not counts.any() and not n_views.any() and inter.shape == (0,) == uni.shape
    head = headtrack.HeadMaps(grid_hw=(5, 9))
    res = head.agreement(c['Rc'], (9, 16), 90.0, np.zeros((0, 3, 3), np.float32), c['offsets'])
    assert res.iou.shape == (0,) and bool(torch.isnan(res.frame_iou).all()) and head.means(res)['frames'] == 0
    assert float(head.coverage(np.zeros((0, 3, 3), np.float32), c['offsets']).abs().max()) == 0.0
