"""The supervised loss (K18) without a GPU: the claims of its restatement (tests/suploss_restate.py) that
tests/test_suploss_gpu.py holds the kernels to - its values are K14's, its analytic gradient is float64 autograd's and a central
difference's - the torch composition the package trains with on the CPU, and the library's exports, status codes and wrappers."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from cp_360_weakly_supervised_saliency_amd import _lib, ops
from cp_360_weakly_supervised_saliency_amd.temporal_model import train_supervised as ts
from cp_360_weakly_supervised_saliency_amd.utils import hashrng
from tests import sphere_eval_restate as rs
from tests import suploss_restate as sr

K18 = ('cp360_sup_loss_work_bytes', 'cp360_sup_loss_forward', 'cp360_sup_loss_backward')
NULL, BAD_SHAPE, ALIGN, UNSUPPORTED = -5, -1, -6, -8
GRIDS = [((5, 9), (12, 24)), ((14, 28), (30, 60)), ((12, 24), (12, 24)), ((32, 64), (12, 24))]
GTERMS = np.array([0.7, -1.3, -0.4])


def noise(seed, *shape):
    return hashrng.uniform(seed, shape, 0.0, 1.0, dtype=np.float64).astype(np.float32)


def one_case(mhw, hw, seed=1800):
    """One map with a unique minimum off the clamped rows, its ground truth and an explicit mask."""
    maps, G, fix = sr.case(seed + mhw[0], 1, mhw[0], mhw[1], hw[0], hw[1])
    return sr.unique_min(maps[0] + 0.3, hw)[None], G, fix


# ----------------------------------------------------------------------------- the restatement's own claims
@pytest.mark.parametrize('mode', ['solid_angle', 'uniform'])
@pytest.mark.parametrize('mhw,hw', GRIDS)
def test_values_are_k14s(mhw, hw, mode):
    maps, G, fix = sr.case(1810, 2, mhw[0], mhw[1], hw[0], hw[1])
    a = rs.weights(hw[0], mode)
    S = rs.resample(maps, *hw)
    for M in (None, fix):
        for n, fw in enumerate(sr.loss(maps, G, a, M)):
            want, n_fix = rs.frame_scores(S[n], G[n], a, None if M is None else M[n])
            assert fw['n'] == n_fix and fw['valid'].all()
            for t, name in enumerate(sr.TERMS):
                assert abs(fw['terms'][t] - want[name]) <= 1e-12 * max(1.0, abs(want[name])), (name, n)


@pytest.mark.parametrize('mhw,hw', GRIDS)
def test_analytic_gradient_is_autograds(mhw, hw):
    """Float64 autograd of the restated forward through the float64 resampler against the analytic gradient at the same S, to
    1e-12 of the map's largest gradient, term by term and combined."""
    maps, G, fix = one_case(mhw, hw)
    a = rs.weights(hw[0])
    _, valid, dm, fws = sr.backward(maps, G, a, GTERMS[None], fix, exact=True)
    assert valid.all()
    m = torch.from_numpy(maps[0].astype(np.float64)).requires_grad_(True)
    terms = sr.torch_terms(m, G[0], a, fix[0], hw)
    for t in range(3):
        want = torch.autograd.grad(terms[t], m, retain_graph=True)[0].numpy()
        got = sr.adjoint(sr.grad_terms(fws[0])[t], *mhw)
        gap = np.max(np.abs(got - want)) / np.max(np.abs(want))
        print('%s -> %s %s: largest gradient %.3e, apart %.2e of it' % (mhw, hw, sr.TERMS[t], np.max(np.abs(want)), gap))
        assert gap <= 1e-12
        assert abs(terms[t].item() - fws[0]['terms'][t]) <= 1e-12
    total = sum(float(GTERMS[t]) * terms[t] for t in range(3))
    want = torch.autograd.grad(total, m)[0].numpy()
    assert np.max(np.abs(dm[0] - want)) <= 1e-12 * np.max(np.abs(want))
    if mhw[0] > hw[0]:                                                 # a map finer than the grid: pixels that no tap touches
        Ry, Rx = sr.matrices(mhw[0], mhw[1], hw[0], hw[1])
        untouched = np.outer(Ry.sum(0) == 0, np.ones(mhw[1], bool)) | np.outer(np.ones(mhw[0], bool), Rx.sum(0) == 0)
        assert untouched.any() and not untouched.all()
        assert np.all(dm[0][untouched] == 0.0) and np.all(want[untouched] == 0.0)


def test_central_difference():
    """5 x 9 -> 12 x 24, every pixel of the small map moved by 1e-6 either way, in float64 through the float64 resampler: the
    difference quotient agrees with the analytic gradient to 1e-6 of the map's largest gradient.  The minimum is unique, by more
    than 1e-3: with 2^-52 in the KL the loss is not smooth where two pixels tie for it."""
    mhw, hw, h = (5, 9), (12, 24), 1e-6
    maps, G, fix = one_case(mhw, hw)
    a = rs.weights(hw[0])
    S = np.sort(sr.resample64(maps[0], *hw).reshape(-1))
    print('gap between the two lowest grid values: %.3e' % (S[1] - S[0]))
    assert S[1] - S[0] > 1e-3
    _, valid, dm, _ = sr.backward(maps, G, a, GTERMS[None], fix, exact=True)
    assert valid.all()
    value = lambda m: float(GTERMS @ sr.loss(m[None], G, a, fix, exact=True)[0]['terms'])
    num = np.zeros(mhw)
    for y in range(mhw[0]):
        for x in range(mhw[1]):
            up, dn = maps[0].astype(np.float64), maps[0].astype(np.float64)
            up[y, x] += h
            dn[y, x] -= h
            num[y, x] = (value(up) - value(dn)) / (2.0 * h)
    gap = np.max(np.abs(num - dm[0])) / np.max(np.abs(dm[0]))
    print('central difference: largest gradient %.3e, apart %.2e of it' % (np.max(np.abs(dm[0])), gap))
    assert gap <= 1e-6


def test_the_first_minimum_is_left_out_of_the_sums():
    """With an eps large enough that nothing cancels (1e-3), K1 and K2 without pixel mm give the gradient that the sums over
    every pixel give after k_mm's terms are taken out again.  Where two pixels tie for the minimum, mm is the lower index: it
    carries the slope of lowering it (the minimum moves with it), the other the slope of raising it (the minimum stays)."""
    h, w, eps = 6, 12, 1e-3
    a = rs.weights(h)
    S = noise(1820, h, w).astype(np.float64) + 0.2
    G = noise(1821, h, w).astype(np.float64)
    S[3, 5] = 0.1
    fw = sr.forward(S, G, a, None, eps)
    assert fw['mm'] == 3 * w + 5
    d = sr.grad_terms(fw)[0]
    k, p, aa, Z, A = fw['k'], fw['p'], fw['a'], fw['Z'], fw['A']
    K1, K2 = (k * p).sum(), (k * aa).sum()                             # over every pixel: p_mm = 0, so K1 is the same
    naive = aa * (k - K1) / Z
    naive[3, 5] = aa[3, 5] * k[3, 5] / Z + ((A - aa[3, 5]) * K1 - K2) / Z   # its own term and the minimum's
    assert np.max(np.abs(naive - d)) <= 1e-12 * np.max(np.abs(d))
    # a tie: pixels (1, 2) and (4, 7)
    S[3, 5] = 0.5
    S[1, 2] = S[4, 7] = 0.1
    fw = sr.forward(S, G, a, None, eps)
    assert fw['mm'] == 1 * w + 2
    d = sr.grad_terms(fw)[0]
    kl = lambda X: sr.forward(X, G, a, None, eps)['terms'][0]
    step = 1e-7
    lower, higher = S.copy(), S.copy()
    lower[1, 2] -= step
    higher[4, 7] += step
    assert abs((kl(S) - kl(lower)) / step - d[1, 2]) <= 1e-5 * np.max(np.abs(d))
    assert abs((kl(higher) - kl(S)) / step - d[4, 7]) <= 1e-5 * np.max(np.abs(d))


def test_invalid_terms_give_no_gradient_and_the_result_is_linear():
    mhw, hw = (5, 9), (12, 24)
    maps, G, fix = sr.case(1830, 4, mhw[0], mhw[1], hw[0], hw[1])
    a = rs.weights(hw[0])
    maps[1] = 0.25                                                     # flat: no variance, no mass
    G[2, 3, 4] = np.nan                                                # a non-finite value: all three
    fix[3] = False                                                     # nothing fixated: NSS
    g = np.tile(GTERMS, (4, 1))
    terms, valid, dm, _ = sr.backward(maps, G, a, g, fix)
    assert valid.tolist() == [[True] * 3, [False] * 3, [False] * 3, [True, True, False]]
    assert np.isnan(terms[~valid]).all() and np.isfinite(terms[valid]).all()
    assert np.all(dm[1] == 0.0) and np.all(dm[2] == 0.0) and np.isfinite(dm).all() and np.any(dm[3] != 0.0)
    only = np.zeros((4, 3))
    parts = []
    for t in range(3):
        only[:] = 0.0
        only[:, t] = g[:, t]
        parts.append(sr.backward(maps, G, a, only, fix)[2])
    assert np.array_equal(parts[2][3], np.zeros(mhw))                  # NSS of map 3 is invalid
    assert np.max(np.abs(parts[0] + parts[1] + parts[2] - dm)) <= 1e-12 * np.max(np.abs(dm))
    assert np.max(np.abs(sr.backward(maps, G, a, -2.0 * g, fix)[2] + 2.0 * dm)) <= 1e-12 * np.max(np.abs(dm))
    assert np.all(sr.backward(maps, G, a, np.zeros((4, 3)), fix)[2] == 0.0)


@pytest.mark.parametrize('with_fix', [False, True])
@pytest.mark.parametrize('mhw,hw', GRIDS)
def test_the_torch_composition_is_the_restatement(mhw, hw, with_fix):
    """supervised_losses_torch in float64 on the CPU: the means over the valid maps and, through autograd, their gradient."""
    B, L = 2, 3
    maps, G, fix = sr.case(1840, B * L, mhw[0], mhw[1], hw[0], hw[1])
    maps = np.stack([sr.unique_min(m + 0.3, hw) for m in maps])
    maps[4] = 0.5                                                      # one invalid map inside the batch
    M = fix if with_fix else None
    a = rs.weights(hw[0])
    g = np.tile(GTERMS / 5.0, (B * L, 1))
    terms, valid, dm, _ = sr.backward(maps, G, a, g, M, exact=True)
    assert valid.sum(0).tolist() == [5, 5, 5]
    m = torch.from_numpy(maps.astype(np.float64)).reshape(B, L, *mhw).requires_grad_(True)
    fx = None if M is None else torch.from_numpy(M).reshape(B, L, *hw)
    kl, cc, nss, counts = ts.supervised_losses_torch(m, torch.from_numpy(G).reshape(B, L, *hw), fx)
    assert counts.tolist() == [5, 5, 5] and counts.dtype == torch.int64
    for t, got in enumerate((kl, cc, nss)):
        want = terms[valid[:, t], t].mean()
        assert abs(got.item() - want) <= 1e-12 * max(1.0, abs(want)), sr.TERMS[t]
    (GTERMS[0] * kl + GTERMS[1] * cc + GTERMS[2] * nss).backward()
    got = m.grad.numpy().reshape(B * L, *mhw)
    assert np.all(got[4] == 0.0)
    assert np.max(np.abs(got - dm)) <= 1e-10 * np.max(np.abs(dm))


def test_the_torch_composition_without_a_valid_map():
    m = torch.full((1, 2, 5, 9), 0.5, dtype=torch.float64, requires_grad=True)
    kl, cc, nss, counts = ts.supervised_losses_torch(m, torch.rand(1, 2, 12, 24, dtype=torch.float64))
    assert counts.tolist() == [0, 0, 0] and kl.item() == 0.0 and cc.item() == 0.0 and nss.item() == 0.0
    assert not kl.requires_grad
    with pytest.raises(ValueError):
        ts.supervised_losses_torch(m, torch.rand(2, 2, 12, 24))
    with pytest.raises(ValueError):
        ts.supervised_losses_torch(m, torch.rand(1, 2, 12, 24), torch.zeros(1, 2, 12, 12, dtype=torch.bool))


def test_the_float32_resampler_in_torch_is_the_restatements():
    src = noise(1850, 3, 14, 28)
    for hw in ((30, 60), (7, 13), (14, 28)):
        assert np.array_equal(ts.resample_torch(torch.from_numpy(src), hw).numpy(), rs.resample(src, *hw))


# ----------------------------------------------------------------------------- library
def test_library_exports_the_symbols():
    L = _lib.lib()
    for name in K18:
        assert name in _lib.PUBLIC_SYMBOLS and hasattr(L, name)
    assert L.cp360_version() == 306 and ops.SUP_LOSS_STATS == 16


def test_status_codes_without_gpu():
    """Argument validation happens before any launch: the dummy pointers are never used."""
    L = _lib.lib()
    one, big, eps = C.c_void_p(16), 1 << 40, 2.0 ** -52
    fwd = lambda *a: L.cp360_sup_loss_forward(*a, None)
    bwd = lambda *a: L.cp360_sup_loss_backward(*a, None)
    ok_f = [one, one, None, one, 2, 5, 9, 12, 24, eps, one, one, one, one, big]
    ok_b = [one, one, None, one, one, one, one, 2, 5, 9, 12, 24, eps, one, one, big]
    for k in (0, 1, 3, 10, 11, 12, 13):
        args = list(ok_f)
        args[k] = None
        assert fwd(*args) == NULL
    for k in (0, 1, 3, 4, 5, 6, 13, 14):
        args = list(ok_b)
        args[k] = None
        assert bwd(*args) == NULL

    def both(N, mh, mw, h, w, e=eps, work=one, nbytes=big):
        f = fwd(one, one, None, one, N, mh, mw, h, w, e, one, one, one, work, nbytes)
        b = bwd(one, one, None, one, one, one, one, N, mh, mw, h, w, e, one, work, nbytes)
        assert f == b
        return f

    for shape in ((0, 5, 9, 12, 24), (2, 0, 9, 12, 24), (2, 5, 0, 12, 24), (2, 5, 9, 0, 24), (2, 5, 9, 12, 0), (-1, 5, 9, 12, 24),
                  (2, 5, -9, 12, 24), (2, 5, 9, 12, -24)):
        assert both(*shape) == BAD_SHAPE and L.cp360_sup_loss_work_bytes(*shape) == 0
    for e in (0.0, -1e-9, math.inf, math.nan):
        assert both(2, 5, 9, 12, 24, e) == BAD_SHAPE
    for shape in ((65536, 5, 9, 12, 24), (1, 5, 9, 1024, 2049), (1, 1024, 2049, 12, 24), (1, 70000, 8, 12, 24)):
        assert both(*shape) == UNSUPPORTED and L.cp360_sup_loss_work_bytes(*shape) == 0
    assert both(0, 5, 9, 1024, 2049) == BAD_SHAPE and both(65536, 5, 9, 12, 24, 0.0) == BAD_SHAPE       # K14's order
    assert L.cp360_sup_loss_work_bytes(1, 1024, 2048, 1024, 2048) > 0
    need = L.cp360_sup_loss_work_bytes(2, 5, 9, 12, 24)
    assert need % 16 == 0 and need >= 2 * 12 * 24 * 12
    assert both(2, 5, 9, 12, 24, nbytes=need - 1) == BAD_SHAPE
    assert both(2, 5, 9, 12, 24, work=C.c_void_p(8)) == ALIGN
    assert fwd(one, one, None, one, 2, 5, 9, 12, 24, eps, C.c_void_p(4), one, one, one, big) == ALIGN
    assert bwd(one, one, None, one, one, one, C.c_void_p(4), 2, 5, 9, 12, 24, eps, one, one, big) == ALIGN
    assert bwd(one, one, None, one, one, one, one, 2, 5, 9, 12, 24, eps, C.c_void_p(2), one, big) == ALIGN


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    m, G = torch.zeros(2, 5, 9), torch.zeros(2, 12, 24)
    wt = ops.sphere_eval_weights(12, 'solid_angle', 'cpu')
    st, va, gt = torch.zeros(2, 16, dtype=torch.float64), torch.zeros(2, 3, dtype=torch.uint8), torch.zeros(2, 3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.sup_loss_forward(m, G, wt)
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.sup_loss_backward(m, G, wt, st, va, gt)
    with pytest.raises(ValueError):
        ops.sup_loss_work(1, (5, 9), (1024, 2049), 'cpu')
    with pytest.raises(ValueError):
        ops.sup_loss_work(1, (0, 9), (12, 24), 'cpu')
    args = ops._sup_loss_args
    assert args(m, G, None, wt, 1e-7) == (2, 5, 9, 12, 24, 1e-7)
    for bad in (lambda: args(m.double(), G, None, wt, 1e-7), lambda: args(m, G[:1], None, wt, 1e-7),
                lambda: args(m, G, None, wt[:5], 1e-7), lambda: args(m, G, None, wt.long(), 1e-7),
                lambda: args(m, G, torch.zeros(2, 12, 24), wt, 1e-7), lambda: args(m, G, torch.zeros(2, 12, 12, dtype=torch.uint8), wt, 1e-7),
                lambda: args(m, G, None, wt, 0.0), lambda: args(m, G, None, wt, float('nan')), lambda: args(m[0], G, None, wt, 1e-7),
                lambda: args(m.transpose(1, 2), G, None, wt, 1e-7)):
        with pytest.raises(ValueError):
            bad()
