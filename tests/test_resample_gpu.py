"""The conservative remap on the sphere (K25, csrc/sphere_resample.hip) on the GPU: the forward bit for bit against the float32
restatement on the library's tables and within the derived bound of float64, on every launch path; non-finite values, batch
independence, out=, a second stream, F = 0; the adjoint; ``DeviceSphereResample`` in front of ``DeviceSupLoss``; the consumers'
opt-in and their unchanged default; and one scene on which the conservative resample is the closer one."""
import functools

import numpy as np
import pytest
import torch

from cp_360_weakly_supervised_saliency_amd import ops
from cp_360_weakly_supervised_saliency_amd.temporal_model import train_supervised as ts
from cp_360_weakly_supervised_saliency_amd.utils import eval_sphere, fixations, hashrng, streaming
from tests import resample_restate as rr

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CASE_IDS = ['%dx%d-%dx%d' % (s + d) for s, d, _ in rr.CASES]


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                       # a copy: the shared cases are read-only


def tables(src_hw, hw):
    return ops.sphere_resample_tables_host(src_hw[0], hw[0], 0), ops.sphere_resample_tables_host(src_hw[1], hw[1], 1)


@functools.lru_cache(maxsize=None)
def case(k):
    """(src float32 [F, hs, ws] in -0.5 .. 1.5, the float32 restatement on the library's tables): made once, shared, read only."""
    src_hw, hw, F = rr.CASES[k]
    src = (hashrng.uniform(2510 + k, (F,) + src_hw, 0.0, 1.0, dtype=np.float64) * 2.0 - 0.5).astype(np.float32)
    want = rr.forward_f32(src, *tables(src_hw, hw))
    src.setflags(write=False)
    want.setflags(write=False)
    return src, want


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


# ----------------------------------------------------------------------------- the forward
@pytest.mark.parametrize('k', range(len(rr.CASES)), ids=CASE_IDS)
def test_forward_is_the_float32_restatement_bit_for_bit(k):
    src_hw, hw, F = rr.CASES[k]
    src, want = case(k)
    got = ops.sphere_resample(dev(src), hw).cpu().numpy()
    assert got.shape == (F,) + hw
    if src_hw[0] > hw[0] or src_hw[1] > hw[1]:
        assert same_bits(got, want)
    # neither axis finer: the bilinear resampler's bits (a copy at equal size), which form a + t (b - a) and no 1 - t
    else:
        assert same_bits(got, ops.sphere_eval_resample(dev(src), hw).cpu().numpy())
        if src_hw == hw:
            assert same_bits(got, src)


@pytest.mark.parametrize('k', range(len(rr.CASES)), ids=CASE_IDS)
def test_forward_within_the_bound_of_float64(k):
    src_hw, hw, F = rr.CASES[k]
    src, _ = case(k)
    ty, tx = tables(src_hw, hw)
    got = ops.sphere_resample(dev(src), hw).cpu().numpy()
    want = rr.forward64(src, hw)
    bound = rr.forward_bound(int(ty[1].max()), int(tx[1].max()), float(np.max(np.abs(src))))
    if not (src_hw[0] > hw[0] or src_hw[1] > hw[1]):
        bound += 4 * 2.0 ** -24 * float(np.max(np.abs(src)))          # a + t (b - a) per axis where the float64 form takes (1 - t) a + t b
    print('kernel - float64: %.3e, bound %.3e' % (np.max(np.abs(got - want)), bound))
    assert np.max(np.abs(got - want)) <= bound
    if src_hw[0] > hw[0] and src_hw[1] > hw[1]:
        assert np.all(np.abs(rr.sphere_integral(got) - rr.sphere_integral(src)) <= 2.0 * bound + 1e-12)


def test_an_offset_source_takes_the_4_byte_loads():
    """A source that starts one element into its buffer: 16-byte loads are illegal, the bits are the same."""
    src, want = case(0)
    buf = torch.zeros(src.size + 1, dtype=torch.float32, device=DEV)
    buf[1:] = dev(src).reshape(-1)
    off = buf[1:].view(src.shape)
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    assert same_bits(ops.sphere_resample(off, rr.CASES[0][1]).cpu().numpy(), want)
    k = 9                                                              # and on the chunked path
    src, want = case(k)
    buf = torch.zeros(src.size + 1, dtype=torch.float32, device=DEV)
    buf[1:] = dev(src).reshape(-1)
    assert same_bits(ops.sphere_resample(buf[1:].view(src.shape), rr.CASES[k][1]).cpu().numpy(), want)


@pytest.mark.parametrize('k', [0, 1, 5, 6], ids=[CASE_IDS[k] for k in (0, 1, 5, 6)])
def test_non_finite_values_show_exactly_where_the_runs_say(k):
    src_hw, hw, F = rr.CASES[k]
    src = case(k)[0].copy()
    hs, ws = src_hw
    src[0, 0, 0], src[0, hs // 2, ws - 1], src[0, hs - 1, ws // 2] = np.nan, np.inf, -np.inf
    src[1, hs // 3, :] = 0.0
    src[1, hs // 3, ws // 3] = np.inf
    src[1, hs // 3 + 1, ws // 3] = -np.inf                             # inf - inf in one run
    src[2] = -np.abs(src[2])
    src[2, :, 0] = 0.0
    ty, tx = tables(src_hw, hw)
    got = ops.sphere_resample(dev(src), hw).cpu().numpy()
    where = rr.nonfinite_where(src, ty, tx)
    assert where[0].any() and where[1].any() and not where[2].any() and not where.all()
    assert np.array_equal(~np.isfinite(got), where)
    want = rr.forward_f32(src, ty, tx)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and same_bits(got[~np.isnan(got)], want[~np.isnan(want)])
    assert np.all(got[2] <= 0)


@pytest.mark.parametrize('k', [0, 1, 5, 10], ids=[CASE_IDS[k] for k in (0, 1, 5, 10)])
def test_a_frame_alone_third_of_five_and_twice(k):
    src_hw, hw, _ = rr.CASES[k]
    frame = case(k)[0][:1]
    five = np.concatenate([case(k)[0][:1] * np.float32(s) for s in (0.5, -1.0, 1.0, 2.0, 0.25)])
    alone = ops.sphere_resample(dev(frame), hw).cpu().numpy()
    batch = dev(five)
    first, again = ops.sphere_resample(batch, hw).cpu().numpy(), ops.sphere_resample(batch, hw).cpu().numpy()
    assert same_bits(first, again) and same_bits(first[2:3], alone) and same_bits(alone, case(k)[1][:1])


def test_out_a_second_stream_and_no_frames():
    src_hw, hw, F = rr.CASES[3]
    src, want = case(3)
    x = dev(src)
    out = torch.full((F,) + hw, 7.0, dtype=torch.float32, device=DEV)
    plan = ops.sphere_resample_plan(src_hw, hw, DEV)
    assert plan is ops.sphere_resample_plan(src_hw, hw, DEV) and plan.dtype == torch.uint8
    assert ops.sphere_resample(x, hw, plan=plan, out=out) is out and same_bits(out.cpu().numpy(), want)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        other = ops.sphere_resample(x, hw)
        back = ops.sphere_resample_adjoint(other, src_hw)
    torch.cuda.current_stream().wait_stream(s)
    assert same_bits(other.cpu().numpy(), want) and same_bits(back.cpu().numpy(), ops.sphere_resample_adjoint(out, src_hw).cpu().numpy())
    none = ops.sphere_resample(torch.zeros((0,) + src_hw, dtype=torch.float32, device=DEV), hw)
    assert tuple(none.shape) == (0,) + hw
    assert tuple(ops.sphere_resample_adjoint(none, src_hw).shape) == (0,) + src_hw
    for call in (lambda: ops.sphere_resample(x, hw, out=out[:, :, :-1]), lambda: ops.sphere_resample(x.double(), hw),
                 lambda: ops.sphere_resample(x, hw, plan=plan[:-16]), lambda: ops.sphere_resample(x[:, :, ::2], hw),
                 lambda: ops.sphere_resample(x, (0, 4)), lambda: ops.sphere_resample_adjoint(out, (16, 40), plan=plan)):
        with pytest.raises(ValueError):
            call()


# ----------------------------------------------------------------------------- the adjoint
@pytest.mark.parametrize('k', range(len(rr.CASES)), ids=CASE_IDS)
def test_adjoint_against_float64_and_the_dot_product_identity(k):
    src_hw, hw, F = rr.CASES[k]
    src, _ = case(k)
    ty, tx = tables(src_hw, hw)
    g = (hashrng.uniform(2540 + k, (F,) + hw, 0.0, 1.0, dtype=np.float64) * 2.0 - 1.0).astype(np.float32)
    got = ops.sphere_resample_adjoint(dev(g), src_hw).cpu().numpy()
    want = rr.adjoint64(g, src_hw, ty, tx)
    # float64 sums rounded once: one float32 rounding of the value, and the float64 roundings of the terms (which may cancel)
    err, mag = np.abs(got.astype(np.float64) - want), rr.adjoint64(np.abs(g), src_hw, ty, tx)
    print('adjoint - float64: %.3e of a float32 rounding at worst' % np.max(err / np.maximum(np.abs(want) * 2.0 ** -24, 1e-300)))
    assert np.all(err <= np.abs(want) * 2.0 ** -24 + mag * 2.0 ** -48 + 2.0 ** -149)
    if src_hw[0] > hw[0] or src_hw[1] > hw[1]:
        fwd = ops.sphere_resample(dev(src), hw).cpu().numpy().astype(np.float64)
        lhs, rhs = np.sum(fwd * g.astype(np.float64)), np.sum(src.astype(np.float64) * got.astype(np.float64))
        scale = np.sum(np.abs(fwd * g)) + np.sum(np.abs(src.astype(np.float64) * got))
        n_y, n_x = int(ty[1].max()), int(tx[1].max())
        # <R m, g> = <m, R^T g>: the forward carries forward_bound's relative error, the adjoint one rounding
        assert abs(lhs - rhs) <= ((1 + rr.U) ** (n_y + n_x + 2) - 1 + rr.U) * scale


def test_a_row_so_long_that_the_adjoints_spans_need_64_bits():
    """ws w >= 2^31: the adjoint finds its grid columns with 64-bit divisions, the forward splits the row over 97 workgroups.  One row
    to one row (the rows' taps are (1, 0) on row 0), so the matrices stay out of memory: the forward against the float32
    restatement, the adjoint against the sum over the tables' entries in float64."""
    (hs, ws), (h, w) = (1, 50000), (1, 45000)
    assert ws * w + ws >= 2 ** 31
    src = hashrng.uniform(2590, (1, hs, ws), 0.0, 1.0, dtype=np.float64).astype(np.float32)
    g = (hashrng.uniform(2591, (1, h, w), 0.0, 1.0, dtype=np.float64) * 2.0 - 1.0).astype(np.float32)
    ty, tx = tables((hs, ws), (h, w))
    assert ty[2].tolist() == [[1.0, 0.0]]
    assert same_bits(ops.sphere_resample(dev(src), (h, w)).cpu().numpy(), rr.forward_f32(src, ty, tx))
    want, mag = np.zeros(ws), np.zeros(ws)
    for k in range(tx[2].shape[1]):
        keep = k < tx[1]
        idx = rr.index_of(tx[0], k, ws, 1)[keep]
        np.add.at(want, idx, tx[2][keep, k].astype(np.float64) * g[0, 0, keep])
        np.add.at(mag, idx, tx[2][keep, k].astype(np.float64) * np.abs(g[0, 0, keep]))
    got = ops.sphere_resample_adjoint(dev(g), (hs, ws)).cpu().numpy().astype(np.float64)[0, 0]
    assert np.all(np.abs(got - want) <= np.abs(want) * 2.0 ** -24 + mag * 2.0 ** -48 + 2.0 ** -149)


# ----------------------------------------------------------------------------- in front of the supervised loss
def test_device_resample_in_front_of_the_loss_matches_the_torch_composition():
    """``supervised_losses(resample='conservative')`` = DeviceSphereResample + DeviceSupLoss against ``supervised_losses_torch``
    with the conservative composition in float64, within tests/test_suploss_gpu.py's tolerances for the bilinear pair: the terms
    within rtol = atol = 1e-6, the gradient within 1e-3 of its largest entry.  kl_eps = 1e-6, as there."""
    B, L, src_hw, hw = 2, 3, (64, 128), (8, 16)
    fy, fx = np.meshgrid(np.arange(src_hw[0]) / 8.0, np.arange(src_hw[1]) / 8.0, indexing='ij')
    maps = 0.3 * hashrng.uniform(2560, (B, L) + src_hw, 0.0, 1.0, dtype=np.float64)
    maps = (maps + np.exp(-((fy - 4.2) ** 2 + (fx - 7.7) ** 2) / 9.0)[None, None]).astype(np.float32)
    yy, xx = np.meshgrid(np.arange(hw[0]), np.arange(hw[1]), indexing='ij')
    gt = np.stack([np.exp(-((yy - 3 - b) ** 2 + (xx - 5 - 2 * t) ** 2) / 6.0) for b in range(B) for t in range(L)])
    gt = gt.reshape(B, L, *hw).astype(np.float32)
    fix = (gt > 0.6).astype(np.uint8)
    out = []
    for device_loss in (True, False):
        x = dev(maps).requires_grad_(True)
        if device_loss:
            kl, cc, nss, counts = ts.supervised_losses(x, dev(gt), dev(fix), kl_eps=1e-6, resample='conservative')
        else:
            x = dev(maps).double().requires_grad_(True)
            kl, cc, nss, counts = ts.supervised_losses_torch(x, dev(gt), dev(fix), kl_eps=1e-6, resample='conservative')
        assert counts.tolist() == [B * L] * 3
        (kl - cc - 0.1 * nss).backward()
        out.append(([v.item() for v in (kl, cc, nss)], x.grad.detach().cpu().numpy().astype(np.float64)))
    (terms, grad), (want_terms, want_grad) = out
    print('terms', terms, 'against', want_terms)
    assert np.allclose(terms, want_terms, rtol=1e-6, atol=1e-6)
    err = float(np.max(np.abs(grad - want_grad)) / np.max(np.abs(want_grad)))
    print('largest gradient %.3e, apart %.2e of it' % (np.max(np.abs(want_grad)), err))
    assert grad.shape == maps.shape and np.max(np.abs(want_grad)) > 0 and err <= 1e-3
    # the bilinear default is untouched: today's call
    a = ts.supervised_losses(dev(maps), dev(gt), dev(fix), kl_eps=1e-6)
    b = ts.supervised_losses(dev(maps), dev(gt), dev(fix), kl_eps=1e-6, resample='bilinear')
    assert [v.item() for v in a[:3]] == [v.item() for v in b[:3]] and a[1].item() != terms[1]


# ----------------------------------------------------------------------------- the consumers
def test_sphere_eval_resamples_conservatively_on_request_and_bilinearly_by_default():
    F, src_hw, hw = 3, (64, 128), (8, 16)
    sal = hashrng.uniform(2570, (F,) + src_hw, 0.0, 1.0, dtype=np.float64).astype(np.float32)
    gt = hashrng.uniform(2571, (F,) + src_hw, 0.0, 1.0, dtype=np.float64).astype(np.float32) ** 4
    plain = eval_sphere.SphereEval(hw, device=DEV)
    S, G = ops.sphere_resample(dev(sal), hw), ops.sphere_resample(dev(gt), hw)
    cons = eval_sphere.SphereEval(hw, device=DEV, resample='conservative')
    assert same_bits(cons.resample(sal).cpu().numpy(), S.cpu().numpy())
    got, want = cons.evaluate(sal, gt), plain.evaluate(S, G)          # by hand first: maps on the grid are copied
    assert np.array_equal(got.scores.cpu().numpy(), want.scores.cpu().numpy(), equal_nan=True)
    assert np.array_equal(got.n_fix.cpu().numpy(), want.n_fix.cpu().numpy())
    today = plain.evaluate(sal, gt)
    by_hand = plain.evaluate(ops.sphere_eval_resample(dev(sal), hw), ops.sphere_eval_resample(dev(gt), hw))
    assert np.array_equal(today.scores.cpu().numpy(), by_hand.scores.cpu().numpy(), equal_nan=True)
    assert same_bits(plain.resample(sal).cpu().numpy(), ops.sphere_eval_resample(dev(sal), hw).cpu().numpy())
    assert not np.array_equal(today.scores.cpu().numpy(), got.scores.cpu().numpy(), equal_nan=True)


def test_fixation_maps_resample_conservatively_on_request():
    F, src_hw, hw = 3, (32, 64), (8, 16)
    sal = hashrng.uniform(2572, (F,) + src_hw, 0.0, 1.0, dtype=np.float64).astype(np.float32)
    lonlat = np.stack([hashrng.uniform(2573, (24,), -3.0, 3.0, dtype=np.float64), hashrng.uniform(2574, (24,), -1.2, 1.2, dtype=np.float64)], 1)
    offsets = np.arange(F + 1, dtype=np.int32) * 8
    plain, cons = fixations.FixationMaps(hw, device=DEV), fixations.FixationMaps(hw, device=DEV, resample='conservative')
    counts = plain.counts(lonlat, offsets)[0]
    S = ops.sphere_resample(dev(sal), hw)
    for a, b in zip(cons.shuffled_auc(sal, counts), plain.shuffled_auc(S, counts)):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True)
    for a, b in zip(plain.shuffled_auc(sal, counts), plain.shuffled_auc(ops.sphere_eval_resample(dev(sal), hw), counts)):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True)
    got, want = cons.score_points(sal, lonlat, offsets), plain.score_points(S, lonlat, offsets)
    assert np.array_equal(got.nss.cpu().numpy(), want.nss.cpu().numpy(), equal_nan=True)
    one, one_want = cons.score_points(sal[0], lonlat, offsets), plain.score_points(S[0], lonlat, offsets)
    assert np.array_equal(one.nss.cpu().numpy(), one_want.nss.cpu().numpy(), equal_nan=True)
    today, by_hand = plain.score_points(sal, lonlat, offsets), plain.score_points(ops.sphere_eval_resample(dev(sal), hw), lonlat, offsets)
    assert np.array_equal(today.nss.cpu().numpy(), by_hand.nss.cpu().numpy(), equal_nan=True)


def test_stream_planner_resamples_conservatively_on_request():
    F, fine, src_hw, grid = 2, (56, 112), (7, 14), (12, 24)
    sal = hashrng.uniform(2575, (F,) + fine, 0.0, 1.0, dtype=np.float64).astype(np.float32) ** 8
    plain = streaming.StreamPlanner(grid, src_hw, tiles=(3, 4), device=DEV)
    cons = streaming.StreamPlanner(grid, src_hw, tiles=(3, 4), device=DEV, resample='conservative')
    by_hand = ops.sphere_resample(dev(sal), src_hw)
    assert same_bits(cons.coverage(sal).cpu().numpy(), plain.coverage(by_hand).cpu().numpy())
    assert same_bits(cons.visibility(sal).cpu().numpy(), plain.visibility(by_hand).cpu().numpy())
    assert same_bits(plain.coverage(sal).cpu().numpy(), plain.coverage(ops.sphere_eval_resample(dev(sal), src_hw)).cpu().numpy())
    assert not same_bits(plain.coverage(sal).cpu().numpy(), cons.coverage(sal).cpu().numpy())


# ----------------------------------------------------------------------------- one scene
def test_on_a_fine_density_the_conservative_resample_is_closer_to_the_block_integral():
    """A fine density at 64 x 128 - three von Mises-Fisher blobs and sparse single-pixel points - against its exact float64
    block integral on 8 x 16: CC is higher for the conservative resample than for the bilinear one.  A comparison, no figure."""
    (hs, ws), (h, w) = (64, 128), (8, 16)
    lat = (0.5 - (np.arange(hs) + 0.5) / hs) * np.pi
    lon = ((np.arange(ws) + 0.5) / ws * 2.0 - 1.0) * np.pi
    d = np.stack([np.cos(lat)[:, None] * np.cos(lon)[None, :], np.repeat(np.sin(lat)[:, None], ws, 1),
                  np.cos(lat)[:, None] * np.sin(lon)[None, :]], -1)
    dens = np.zeros((hs, ws))
    for (la, lo, kappa, amp) in ((0.3, -2.0, 40.0, 1.0), (-0.6, 0.4, 90.0, 0.7), (1.1, 2.6, 25.0, 0.5)):
        c = np.array([np.cos(la) * np.cos(lo), np.sin(la), np.cos(la) * np.sin(lo)])
        dens += amp * np.exp(kappa * (d @ c - 1.0))
    ys = hashrng.uniform(2580, (40,), 0.0, 1.0, dtype=np.float64)
    xs = hashrng.uniform(2581, (40,), 0.0, 1.0, dtype=np.float64)
    dens[(ys * hs).astype(int), (xs * ws).astype(int)] += 3.0
    a = rr.band(hs)
    truth = (dens * a[:, None]).reshape(h, hs // h, w, ws // w).sum(axis=(1, 3)) / (a.reshape(h, hs // h).sum(axis=1)[:, None] * (ws // w))
    x = dev(dens.astype(np.float32)[None])
    cons = ops.sphere_resample(x, (h, w)).cpu().numpy()[0].astype(np.float64)
    bil = ops.sphere_eval_resample(x, (h, w)).cpu().numpy()[0].astype(np.float64)

    def cc(m):
        wgt = np.repeat(rr.band(h)[:, None], w, 1)
        mm, tt = m - np.sum(wgt * m) / wgt.sum(), truth - np.sum(wgt * truth) / wgt.sum()
        return np.sum(wgt * mm * tt) / np.sqrt(np.sum(wgt * mm * mm) * np.sum(wgt * tt * tt))

    print('CC against the block integral: conservative %.6f, bilinear %.6f' % (cc(cons), cc(bil)))
    assert cc(cons) > cc(bil)
