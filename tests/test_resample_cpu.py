"""The conservative remap on the sphere (K25) without a GPU: the claims of the restatement (tests/resample_restate.py) that
tests/test_resample_gpu.py holds the kernels to, the library's host tables against it, the flaw of the bilinear resampler that
the feature removes, the torch composition and its gradient, and the exports, status codes and refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

from cp_360_weakly_supervised_saliency_amd import _lib, ops
from cp_360_weakly_supervised_saliency_amd.temporal_model import train_supervised as ts
from cp_360_weakly_supervised_saliency_amd.utils import eval_sphere, fixations, hashrng, streaming
from tests import resample_restate as rr

K25 = ('cp360_sresample_run_cap', 'cp360_sresample_axis_host', 'cp360_sresample_plan_bytes', 'cp360_sresample_plan_host',
       'cp360_sresample_forward', 'cp360_sresample_adjoint')
NULL, BAD_SHAPE, ALIGN, UNSUPPORTED = -5, -1, -6, -8
# the five shapes the definition was first checked on, a mixed pair each way and an upsampling pair
SHAPES = [((64, 128), (8, 16)), ((45, 91), (7, 13)), ((33, 64), (32, 60)), ((16, 32), (5, 9)), ((100, 37), (3, 36)),
          ((40, 16), (8, 32)), ((6, 96), (12, 24))]
AXES = sorted({(s[a], d[a], a) for s, d, _ in rr.CASES for a in (0, 1)} | {(s[a], d[a], a) for s, d in SHAPES for a in (0, 1)})


def noise(seed, *shape):
    return hashrng.uniform(seed, shape, 0.0, 1.0, dtype=np.float64)


# ----------------------------------------------------------------------------- the runs: integer facts
@pytest.mark.parametrize('n_src,n_dst,axis', [a for a in AXES if a[0] > a[1]])
def test_runs_are_contiguous_cover_the_axis_and_weigh_positive(n_src, n_dst, axis):
    start, count, weights, ov = rr.axis_tables(n_src, n_dst, axis)
    assert np.all(count >= 1) and np.all(count <= rr.run_cap(n_src, n_dst))
    assert start[0] == 0 and start[-1] + count[-1] == n_src                       # never wrapping, the whole axis
    assert np.all(start[1:] <= start[:-1] + count[:-1]) and np.all(start[1:] >= start[:-1] + count[:-1] - 1)   # no gap, at most one shared
    for d in range(n_dst):
        assert np.all(weights[d, :count[d]] > 0) and np.all(weights[d, count[d]:] == 0)
    if axis == 1:
        assert np.all(ov.sum(axis=1) == n_src)                                   # the overlaps of a run: exact integers that sum to ws
        hit = np.zeros(n_src, np.int64)
        for d in range(n_dst):
            hit[start[d]:start[d] + count[d]] += ov[d, :count[d]]
        assert np.all(hit == n_dst)                                              # every source column is read, all of it
    else:
        assert np.allclose(rr.dense(start, count, weights, n_src, 0).T @ rr.band(n_dst), rr.band(n_src), rtol=1e-12, atol=0)


# ----------------------------------------------------------------------------- the library's tables
@pytest.mark.parametrize('n_src,n_dst,axis', AXES)
def test_host_tables_match_the_restatement(n_src, n_dst, axis):
    start, count, weights = ops.sphere_resample_tables_host(n_src, n_dst, axis)
    R = rr.run_cap(n_src, n_dst)
    assert _lib.lib().cp360_sresample_run_cap(n_src, n_dst) == R
    assert start.dtype == count.dtype == np.int32 and weights.dtype == np.float32 and weights.shape == (n_dst, R)
    s64, c64, w64, _ = rr.axis_tables(n_src, n_dst, axis)
    assert np.array_equal(start, s64) and np.array_equal(count, c64)
    if n_src > n_dst:
        err = np.abs(weights.astype(np.float64) - w64)
        print('largest weight error / weight: %.3e (one rounding: %.3e)' % (np.max(err[w64 > 0] / w64[w64 > 0]), rr.U))
        assert np.all(err <= rr.TAB_REL * w64)
    else:
        assert np.array_equal(weights, w64.astype(np.float32))                   # the taps are float32 by definition
        i0, t = rr.taps(n_src, n_dst, axis)
        assert np.array_equal(weights[:, 1], t) and np.array_equal(weights[:, 0], (np.float32(1) - t).astype(np.float32))
    for d in range(n_dst):
        assert np.all(weights[d, count[d]:] == 0)
    assert np.all(np.abs(weights.astype(np.float64).sum(axis=1) - 1.0) <= R * 2.0 ** -24)


def test_tapped_tables_are_the_bilinear_resamplers_taps():
    for n_src, n_dst, axis in [(14, 60, 1), (7, 30, 0), (9, 9, 1), (5, 5, 0), (16, 32, 1)]:
        start, count, weights = ops.sphere_resample_tables_host(n_src, n_dst, axis)
        i0, i1, t = ts._taps(n_dst, n_src, axis == 1)
        assert np.array_equal(start, i0) and np.all(count == 2) and np.array_equal(weights[:, 1], t)
        assert np.array_equal(rr.index_of(start, 1, n_src, axis), i1)


# ----------------------------------------------------------------------------- the definition in float64
@pytest.mark.parametrize('src_hw,hw', SHAPES)
def test_constant_integral_and_adjoint_identity_in_float64(src_hw, hw):
    both = src_hw[0] > hw[0] and src_hw[1] > hw[1]
    m = noise(2501, 2, *src_hw)
    out = rr.forward64(m, hw)
    # a constant stays: to float64 rounding where both axes are conservative; a tapped axis' float32 weights (1 - t, t) may miss 1
    # by a float32 rounding
    assert np.max(np.abs(rr.forward64(np.full((1,) + src_hw, 0.7), hw) - 0.7)) <= (8 * 2.0 ** -53 if both else 2.0 ** -24)
    if both:
        got, want = rr.sphere_integral(out), rr.sphere_integral(m)
        print('integral', got, 'against', want)
        assert np.all(np.abs(got - want) <= 1e-13 * np.abs(want))
    g = noise(2502, 2, *hw)
    ty, tx = rr.axis_tables(src_hw[0], hw[0], 0)[:3], rr.axis_tables(src_hw[1], hw[1], 1)[:3]
    lhs, rhs = np.sum(out * g), np.sum(m * rr.adjoint64(g, src_hw, ty, tx))
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs)


def test_an_integer_ratio_is_the_weighted_block_mean():
    (hs, ws), (h, w), k = (64, 128), (8, 16), 8
    m = noise(2503, 1, hs, ws)
    a = rr.band(hs)
    blocks = (m[0] * a[:, None]).reshape(h, k, w, k).sum(axis=(1, 3)) / (a.reshape(h, k).sum(axis=1)[:, None] * k)
    assert np.max(np.abs(rr.forward64(m, (h, w))[0] - blocks)) <= 1e-14
    s, c, _, _ = rr.axis_tables(hs, h, 0)
    assert np.all(c == k) and np.array_equal(s, np.arange(h) * k)                # the runs are the blocks: no shared row


@pytest.mark.parametrize('src_hw,hw', [s for s in SHAPES if s[0][0] > s[1][0] and s[0][1] > s[1][1]])
def test_every_one_hot_source_keeps_its_solid_angle(src_hw, hw):
    """A source of one pixel, at every position: the output's mass on the sphere is that pixel's solid angle."""
    (hs, ws), (h, w) = src_hw, hw
    Wy = rr.dense(*rr.axis_tables(hs, h, 0)[:3], hs, 0)
    Wx = rr.dense(*rr.axis_tables(ws, w, 1)[:3], ws, 1)
    mass = np.einsum('y,yr,xj->rj', rr.band(h), Wy, Wx) / w                      # [hs, ws]: the mass of the one-hot at (r, j)
    want = np.repeat(rr.band(hs)[:, None] / ws, ws, axis=1)
    assert np.all(mass > 0) and np.max(np.abs(mass - want) / want) <= 1e-12
    one = np.zeros((1, hs, ws))
    one[0, hs // 3, ws - 1] = 1.0                                                # and once through forward64 itself
    assert abs(rr.sphere_integral(rr.forward64(one, hw))[0] - want[hs // 3, ws - 1]) <= 1e-12 * want[hs // 3, ws - 1]


def test_the_bilinear_resampler_loses_fifteen_sixteenths_of_the_one_hot_sources():
    """The flaw the feature removes: at ratio 8 the four bilinear taps read 4 of every 64 source pixels, so a one-pixel source
    leaves no mass at all from 15/16 of the positions; the conservative remap keeps every one."""
    (hs, ws), (h, w) = (64, 128), (8, 16)
    lost_bilinear = lost_conservative = 0
    for r0 in range(0, hs, 8):
        one = torch.zeros((8 * ws, hs, ws), dtype=torch.float32)
        one.view(8, ws, hs, ws)[torch.arange(8)[:, None], torch.arange(ws)[None, :], r0 + torch.arange(8)[:, None],
                                torch.arange(ws)[None, :]] = 1.0
        lost_bilinear += int((ts.resample_torch(one, (h, w)).abs().sum(dim=(1, 2)) == 0).sum())
        lost_conservative += int((ts.resample_conservative_torch(one, (h, w)).abs().sum(dim=(1, 2)) == 0).sum())
    assert lost_bilinear == hs * ws * 15 // 16
    assert lost_conservative == 0


# ----------------------------------------------------------------------------- the float32 form and its bound
@pytest.mark.parametrize('src_hw,hw', SHAPES)
def test_float32_restatement_within_its_bound_of_float64(src_hw, hw):
    m = (noise(2504, 2, *src_hw) * 2.0 - 0.5).astype(np.float32)
    ty, tx = ops.sphere_resample_tables_host(src_hw[0], hw[0], 0), ops.sphere_resample_tables_host(src_hw[1], hw[1], 1)
    got, want = rr.forward_f32(m, ty, tx), rr.forward64(m, hw)
    bound = rr.forward_bound(int(ty[1].max()), int(tx[1].max()), float(np.max(np.abs(m))))
    print('float32 - float64: %.3e, bound %.3e' % (np.max(np.abs(got - want)), bound))
    assert np.max(np.abs(got - want)) <= bound
    if src_hw[0] > hw[0] and src_hw[1] > hw[1]:
        c = rr.forward_f32(np.full((1,) + src_hw, 0.7, np.float32), ty, tx)
        assert np.max(np.abs(c - np.float32(0.7))) <= rr.forward_bound(int(ty[1].max()), int(tx[1].max()), 0.7)
        mass = rr.sphere_integral(got)
        assert np.all(np.abs(mass - rr.sphere_integral(m)) <= 2.0 * bound + 1e-12)      # the bands sum to 2
        bad = m.copy()
        bad[0, 3, 5], bad[1, src_hw[0] - 1, 0] = np.nan, np.inf
        assert np.array_equal(~np.isfinite(rr.forward_f32(bad, ty, tx)), rr.nonfinite_where(bad, ty, tx))


# ----------------------------------------------------------------------------- the torch composition
@pytest.mark.parametrize('src_hw,hw', SHAPES + [((7, 14), (30, 60)), ((5, 9), (5, 9))])
def test_torch_composition_and_its_gradient(src_hw, hw):
    m = torch.from_numpy(noise(2505, 2, *src_hw)).requires_grad_(True)
    out = ts.resample_conservative_torch(m, hw)
    assert out.dtype == torch.float64 and tuple(out.shape) == (2,) + hw
    ty, tx = ops.sphere_resample_tables_host(src_hw[0], hw[0], 0), ops.sphere_resample_tables_host(src_hw[1], hw[1], 1)
    Wy = rr.dense(ty[0], ty[1], ty[2].astype(np.float64), src_hw[0], 0)
    Wx = rr.dense(tx[0], tx[1], tx[2].astype(np.float64), src_hw[1], 1)
    want = np.einsum('yr,frj,xj->fyx', Wy, m.detach().numpy(), Wx)
    assert np.max(np.abs(out.detach().numpy() - want)) <= 1e-14
    assert np.max(np.abs(want - rr.forward64(m.detach().numpy(), hw))) <= 4 * rr.TAB_REL     # the library's weights are rounded
    g = noise(2506, 2, *hw)
    out.backward(torch.from_numpy(g))
    assert np.max(np.abs(m.grad.numpy() - rr.adjoint64(g, src_hw, ty, tx))) <= 1e-14
    if not (src_hw[0] > hw[0] or src_hw[1] > hw[1]):
        # neither axis finer: the bilinear taps as a matrix, whose 1 - t is rounded to float32 where a + t (b - a) forms none:
        # a rounding per axis on values below 1
        assert np.max(np.abs(out.detach().numpy() - ts.resample_torch(m.detach(), hw).numpy())) <= 2 * 2.0 ** -24


def test_supervised_losses_torch_takes_the_conservative_composition():
    maps = torch.from_numpy(noise(2507, 1, 2, 32, 64))
    gt = torch.from_numpy(noise(2508, 1, 2, 8, 16))
    a = ts.supervised_losses_torch(maps, gt, resample='conservative')
    b = ts.supervised_losses_torch(ts.resample_conservative_torch(maps[0], (8, 16))[None], gt)
    c = ts.supervised_losses_torch(maps, gt)
    assert [v.item() for v in a[:3]] == [v.item() for v in b[:3]] and a[1].item() != c[1].item()


# ----------------------------------------------------------------------------- exports, status codes, refusals
def test_exports_at_version_306():
    L = _lib.lib()
    assert all(hasattr(L, n) for n in K25) and set(K25) <= set(_lib.PUBLIC_SYMBOLS)
    assert L.cp360_version() == _lib.ABI_VERSION == 306


def test_status_codes_without_a_gpu():
    L = _lib.lib()
    one, odd = C.c_void_p(4096), C.c_void_p(4098)
    assert L.cp360_sresample_run_cap(0, 4) == 0 and L.cp360_sresample_run_cap(4, 0) == 0
    assert L.cp360_sresample_run_cap(64, 8) == 9 and L.cp360_sresample_run_cap(65, 8) == 10 and L.cp360_sresample_run_cap(8, 8) == 2
    assert L.cp360_sresample_axis_host(64, 8, 0, None, one, one) == NULL
    assert L.cp360_sresample_axis_host(64, 0, 0, one, one, one) == BAD_SHAPE
    assert L.cp360_sresample_axis_host(64, 8, 2, one, one, one) == BAD_SHAPE
    assert L.cp360_sresample_axis_host(2041, 8, 0, one, one, one) == UNSUPPORTED                # a run of 257
    assert L.cp360_sresample_plan_bytes(64, 128, 8, 16) > 0 and L.cp360_sresample_plan_bytes(2040, 128, 8, 16) > 0
    assert L.cp360_sresample_plan_bytes(2041, 128, 8, 16) == 0 and L.cp360_sresample_plan_bytes(64, 4081, 8, 16) == 0
    assert L.cp360_sresample_plan_bytes(0, 128, 8, 16) == 0
    assert L.cp360_sresample_plan_host(64, 128, 8, 16, None, 1 << 20) == NULL
    assert L.cp360_sresample_plan_host(64, 128, 8, 16, odd, 1 << 20) == ALIGN
    assert L.cp360_sresample_plan_host(64, 128, 8, 16, one, 16) == BAD_SHAPE
    need = L.cp360_sresample_plan_bytes(64, 128, 8, 16)
    for fn, a, b in ((L.cp360_sresample_forward, (64, 128), (8, 16)), (L.cp360_sresample_adjoint, (8, 16), (64, 128))):
        call = lambda src, F, dst, plan, n, a=a, b=b: fn(src, F, a[0], a[1], dst, b[0], b[1], plan, n, None)
        assert call(None, 2, one, one, need) == NULL and call(one, 2, None, one, need) == NULL and call(one, 2, one, None, need) == NULL
        assert call(one, -1, one, one, need) == BAD_SHAPE
        assert fn(one, 2, 0, a[1], one, b[0], b[1], one, need, None) == BAD_SHAPE
        assert call(one, 65536, one, one, need) == UNSUPPORTED
        assert call(odd, 2, one, one, need) == ALIGN and call(one, 2, odd, one, need) == ALIGN
        assert call(one, 2, one, C.c_void_p(4100), need) == ALIGN
        assert call(one, 2, one, one, need - 1) == BAD_SHAPE
        assert call(None, 0, None, one, need) == 0                                # F = 0: nothing to launch
        assert call(None, 0, None, one, need - 1) == BAD_SHAPE                    # ... after every check
    # the order: NULL, shape, unsupported, alignment, workspace
    assert L.cp360_sresample_forward(None, 2, 0, 128, odd, 8, 16, one, 0, None) == NULL
    assert L.cp360_sresample_forward(odd, 2, 0, 128, odd, 8, 16, one, 0, None) == BAD_SHAPE
    assert L.cp360_sresample_forward(odd, 2, 2041, 128, odd, 8, 16, one, 0, None) == UNSUPPORTED      # the run cap
    assert L.cp360_sresample_forward(odd, 2, 64, 4081, one, 8, 16, one, 0, None) == UNSUPPORTED
    assert L.cp360_sresample_forward(odd, 2, 64, 128, one, 8, 16, one, 0, None) == ALIGN
    assert L.cp360_sresample_forward(one, 2, 64, 128, one, 1024, 2049, one, need, None) == UNSUPPORTED   # cp360_seval_resample's limits
    assert L.cp360_sresample_forward(one, 2, 70000, 8, one, 8, 16, one, need, None) == UNSUPPORTED


def test_the_wrappers_refuse():
    cpu = torch.zeros((2, 64, 128))
    for call in (lambda: ops.sphere_resample(cpu, (8, 16)), lambda: ops.sphere_resample_adjoint(torch.zeros((2, 8, 16)), (64, 128)),
                 lambda: ops.sphere_resample_plan((64, 128), (8, 16), 'cpu')):
        with pytest.raises(RuntimeError, match='GPU only'):
            call()
    for call in (lambda: ops.sphere_resample_tables_host(0, 4, 0), lambda: ops.sphere_resample_tables_host(8, 4, 2),
                 lambda: ops.sphere_resample_tables_host(2041, 8, 0), lambda: ops.check_resampler('lanczos'),
                 lambda: ops.sphere_resample_plan((0, 128), (8, 16), 'cuda'),
                 lambda: ops.sphere_resample_plan((2041, 128), (8, 16), 'cuda')):
        with pytest.raises(ValueError):
            call()
    assert ops.check_resampler('bilinear') == 'bilinear' and ops.check_resampler('conservative') == 'conservative'


def test_every_consumer_refuses_an_unknown_resampler():
    maps, gt = torch.zeros((1, 2, 16, 32)), torch.zeros((1, 2, 8, 16))
    for call in (lambda: eval_sphere.SphereEval(resample='nearest'), lambda: fixations.FixationMaps(resample='nearest'),
                 lambda: streaming.StreamPlanner(resample='nearest'), lambda: ts.supervised_losses(maps, gt, resample='nearest'),
                 lambda: ts.supervised_losses_torch(maps, gt, resample='nearest')):
        with pytest.raises(ValueError, match="resample must be 'bilinear' or 'conservative'"):
            call()
    assert eval_sphere.SphereEval().resampler == 'bilinear' and fixations.FixationMaps().resampler == 'bilinear'
    assert streaming.StreamPlanner().resampler == 'bilinear'
    assert eval_sphere.SphereEval(resample='conservative').resampler == 'conservative'
