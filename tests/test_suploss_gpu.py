"""The supervised loss on the GPU (K18, csrc/suploss.hip) against its float64 restatement (tests/suploss_restate.py, whose own
claims tests/test_suploss_cpu.py pins) and against K14 itself.

Tolerances.  The terms are K14's sums: tests/test_sphere_eval_gpu.py's 1e-9, relative or absolute, for nss, cc and kl.  The
gradient is float64 sums in a fixed order, rounded to float32 once: |d| <= 2^-23 |want| + 1e-9 max|want| per map, the one
rounding of the store (half an ulp: 2^-24) plus the order of the float64 sums.  Measured on the MI355X: DESIGN.md "K18".
valid, mm and n_fix are decisions on float32 values compared in double: exact."""
import functools
import math
import types

import numpy as np
import pytest
import torch

from cp_360_weakly_supervised_saliency_amd import _lib, ops
from cp_360_weakly_supervised_saliency_amd.model.clstm import ConvLSTMCell
from cp_360_weakly_supervised_saliency_amd.model.clstm_train import window_maps
from cp_360_weakly_supervised_saliency_amd.temporal_model import train_supervised as ts
from cp_360_weakly_supervised_saliency_amd.temporal_model.train_temporal import FusedAdam, normalize_batch
from cp_360_weakly_supervised_saliency_amd.utils import eval_sphere, fixations, hashrng, synth
from tests import sphere_eval_restate as rs
from tests import suploss_restate as sr

pytestmark = pytest.mark.gpu
DEV = 'cuda'
EPS = 2.0 ** -52
GRIDS = [((5, 9), (12, 24)),          # P = 288: below the 1024 threads
         ((14, 28), (120, 240)),      # the training shape: 29 passes of the workgroup, 113 blocks of K18b
         ((12, 24), (12, 24)),        # the copy path
         ((32, 64), (12, 24)),        # a map finer than the grid: small pixels that no tap touches
         ((3, 4), (7, 13))]           # odd sizes
ST_MM, ST_N = 10, 11
N = 5


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a, order='C')).to(DEV)


def wt(h, mode='solid_angle'):
    return ops.sphere_eval_weights(h, mode, torch.device(DEV, torch.cuda.current_device()))


def gterms_of(n, seed=1900):
    return hashrng.uniform(seed, (n, 3), -1.5, 1.5, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def case(mhw, hw):
    """(maps, G, fix) of N maps, read-only: shared by the tests of a grid."""
    out = sr.case(1900 + mhw[0], N, mhw[0], mhw[1], hw[0], hw[1])
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def restated(mhw, hw, mode, with_fix):
    """The restatement's (terms, valid, dmaps, forward results) of case(mhw, hw) with gterms_of(N)."""
    maps, G, fix = case(mhw, hw)
    return sr.backward(maps, G, rs.weights(hw[0], mode), gterms_of(N), fix if with_fix else None)


def run(maps, G, fix, mode='solid_angle', eps=EPS, gterms=None, work=None):
    """-> (terms, valid, stats, dmaps) as numpy arrays."""
    m, g, fx, a = dev(maps), dev(G), dev(fix), wt(G.shape[1], mode)
    terms, valid, stats = ops.sup_loss_forward(m, g, a, fx, eps, work=work)
    assert terms.shape == (len(maps), 3) and terms.dtype == torch.float64 and valid.dtype == torch.uint8 and stats.shape[1] == 16
    gt = dev(gterms_of(len(maps)) if gterms is None else gterms)
    dm = ops.sup_loss_backward(m, g, a, stats, valid, gt, fx, eps, work=work)
    assert dm.shape == m.shape and dm.dtype == torch.float32
    return terms.cpu().numpy(), valid.cpu().numpy(), stats.cpu().numpy(), dm.cpu().numpy()


def assert_terms(got, want, what=''):
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    for n in range(want.shape[0]):
        for t, name in enumerate(sr.TERMS):
            if math.isnan(want[n, t]):
                continue
            err = abs(got[n, t] - want[n, t])
            print('%s map %d %s: %.15g against %.15g, apart %.2e' % (what, n, name, got[n, t], want[n, t], err))
            assert err <= 1e-9 * max(1.0, abs(want[n, t])), (n, name)


def assert_grad(got, want, what='', slack=None):
    """slack [N]: what the restatement itself is uncertain by (test_a_minimum_in_the_top_row_ties_grid_pixels)."""
    assert got.shape == want.shape and np.isfinite(got).all()
    for n in range(want.shape[0]):
        top = np.max(np.abs(want[n]))
        d = np.abs(got[n].astype(np.float64) - want[n])
        extra = 0.0 if slack is None else slack[n]
        print('%s map %d gradient: max|want| %.3e, apart at most %.2e of it%s' % (what, n, top, np.max(d) / max(top, 1e-300),
                                                                            '' if slack is None else ' (slack %.2e of it)' % (extra / top)))
        assert np.all(d <= 2.0 ** -23 * np.abs(want[n]) + 1e-9 * top + extra), n


# ----------------------------------------------------------------------------- forward and backward against the restatement
@pytest.mark.parametrize('with_fix', [False, True])
@pytest.mark.parametrize('mode', ['solid_angle', 'uniform'])
@pytest.mark.parametrize('mhw,hw', GRIDS)
def test_terms_and_gradient_match_the_restatement_and_k14(mhw, hw, mode, with_fix):
    maps, G, fix = case(mhw, hw)
    fix = fix if with_fix else None
    want_terms, want_valid, want_dm, fws = restated(mhw, hw, mode, with_fix)
    assert want_valid.all()
    terms, valid, stats, dm = run(maps, G, fix, mode)
    assert np.array_equal(valid != 0, want_valid)
    assert_terms(terms, want_terms, 'restatement')
    assert stats[:, ST_MM].tolist() == [fw['mm'] for fw in fws] and stats[:, ST_N].tolist() == [fw['n'] for fw in fws]
    assert_grad(dm, want_dm)
    # K14 itself, through its own two calls
    S = ops.sphere_eval_resample(dev(maps), hw)
    scores, n_fix = ops.sphere_eval(S, dev(G), wt(hw[0], mode), dev(fix))
    assert_terms(terms, scores.cpu().numpy()[:, [4, 2, 1]], 'K14')
    assert n_fix.cpu().tolist() == stats[:, ST_N].tolist()
    # N = 1: the first map alone is the first map of the batch, bit for bit
    t1, v1, s1, d1 = run(maps[:1], G[:1], None if fix is None else fix[:1], mode, gterms=gterms_of(N)[:1])
    assert np.array_equal(t1, terms[:1]) and np.array_equal(v1, valid[:1]) and np.array_equal(s1, stats[:1])
    assert np.array_equal(d1, dm[:1])
    if mhw[0] > hw[0]:
        Ry, Rx = sr.matrices(mhw[0], mhw[1], hw[0], hw[1])
        untouched = np.outer(Ry.sum(0) == 0, np.ones(mhw[1], bool)) | np.outer(np.ones(mhw[0], bool), Rx.sum(0) == 0)
        assert untouched.any() and np.all(dm[:, untouched] == 0.0) and not np.signbit(dm[:, untouched]).any()


# ----------------------------------------------------------------------------- edges
def test_invalid_maps_leave_their_neighbours_alone():
    """The first, a middle and the last map of a batch made invalid in turn (a flat map; a NaN in G; an infinity in the map): K14's
    NaN, valid = 0, a gradient of exactly +0, and the other maps' bits unchanged."""
    mhw, hw = (5, 9), (12, 24)
    maps, G, fix = case(mhw, hw)
    base = run(maps, G, fix)
    for n in (0, 2, N - 1):
        for kind in ('flat', 'nan', 'inf'):
            m, g = maps.copy(), G.copy()
            if kind == 'flat':
                m[n] = 0.5
            elif kind == 'nan':
                g[n, 5, 7] = np.nan
            else:
                m[n, 2, 3] = np.inf
            terms, valid, _, dm = run(m, g, fix)
            want = sr.backward(m, g, rs.weights(hw[0]), gterms_of(N), fix)
            assert not valid[n].any() and np.isnan(terms[n]).all() and np.isnan(want[0][n]).all()
            assert np.all(dm[n] == 0.0) and not np.signbit(dm[n]).any()
            keep = [k for k in range(N) if k != n]
            assert np.array_equal(terms[keep], base[0][keep]) and np.array_equal(dm[keep], base[3][keep])
            assert valid[keep].all()
            sc = ops.sphere_eval(ops.sphere_eval_resample(dev(m), hw), dev(g), wt(hw[0]), dev(fix))[0].cpu().numpy()
            assert np.array_equal(np.isnan(sc[:, [4, 2, 1]]), np.isnan(terms))


def test_degenerate_ground_truth_and_masks():
    mhw, hw = (5, 9), (12, 24)
    maps, G, fix = case(mhw, hw)
    a = rs.weights(hw[0])
    # G of all zeros: no variance and no mass in G (KL, CC) and an empty derived mask (NSS)
    terms, valid, _, dm = run(maps, np.zeros_like(G), None)
    assert not valid.any() and np.isnan(terms).all() and np.all(dm == 0.0)
    # an explicit mask of all zeros / all ones: NSS alone is undefined
    for value in (0, 1):
        fx = np.full(G.shape, value, np.uint8)
        terms, valid, _, dm = run(maps, G, fx)
        want = sr.backward(maps, G, a, gterms_of(N), fx != 0)
        assert valid.tolist() == [[1, 1, 0]] * N and np.array_equal(want[1], valid != 0)
        assert np.isnan(terms[:, 2]).all()
        assert_terms(terms, want[0])
        assert_grad(dm, want[2])


def test_a_gterms_column_of_zeros_and_linearity():
    mhw, hw = (5, 9), (12, 24)
    maps, G, fix = case(mhw, hw)
    a = rs.weights(hw[0])
    g = gterms_of(N)
    full = run(maps, G, fix, gterms=g)[3]
    parts = []
    for t in range(3):
        only = np.zeros_like(g)
        only[:, t] = g[:, t]
        parts.append(run(maps, G, fix, gterms=only)[3])
        assert_grad(parts[t], sr.backward(maps, G, a, only, fix)[2], sr.TERMS[t])
        off = g.copy()
        off[:, t] = 0.0
        assert_grad(run(maps, G, fix, gterms=off)[3], sr.backward(maps, G, a, off, fix)[2], 'without ' + sr.TERMS[t])
    assert np.all(run(maps, G, fix, gterms=np.zeros_like(g))[3] == 0.0)
    total = parts[0].astype(np.float64) + parts[1] + parts[2]
    top = np.max(np.abs(np.stack(parts + [full])), axis=(0, 2, 3))[:, None, None]
    assert np.all(np.abs(total - full) <= 2.0 ** -22 * top)           # four float32 roundings, half an ulp of the largest each
    twice = run(maps, G, fix, gterms=2.0 * g)[3]
    assert np.array_equal(twice, 2.0 * full)                          # a power of two: exact


@pytest.mark.parametrize('mhw,hw', [((4, 8), (16, 32)), ((14, 28), (120, 240))])
def test_a_minimum_in_the_top_row_ties_grid_pixels(mhw, hw):
    """Rows clamp: the grid rows above the first source row's centre repeat it (two of them at a ratio of 4, four at the training
    shape's 8.6), so a minimum there is held by several grid pixels.  mm is the lowest index among them, as the restatement
    names it.  The gradient's gate has one more term here.  A tied pixel j has P_j = 0 and k_j of the order Q_j / eps, about 1e10
    times a typical k; it enters dS_j as a_j k_j / Z and dS_mm, through K2, as -a_j k_j / Z, and the two meet again in the small
    pixel both sample, where they cancel.  What is left carries the rounding of K2, a float64 sum of P terms: (log2 P + 4) 2^-53
    sum_i |k_i a_i| / Z |gterms_kl| in the kernel's tree and as much in numpy's pairwise sum.  That is the restatement's own
    uncertainty, computed from its k, a and Z - not from the kernel's output."""
    maps, G, fix = case(mhw, hw)
    m = maps.copy()
    m[:, 0, 3] = -1.0
    a = rs.weights(hw[0])
    want = sr.backward(m, G, a, gterms_of(N), fix)
    S = rs.resample(m, *hw)
    assert all((S[n] == S[n].min()).sum() >= 2 for n in range(N))
    terms, valid, stats, dm = run(m, G, fix)
    assert stats[:, ST_MM].tolist() == [fw['mm'] for fw in want[3]] and all(fw['mm'] < hw[1] for fw in want[3])
    assert np.array_equal(valid != 0, want[1])
    assert_terms(terms, want[0])
    P, g = hw[0] * hw[1], gterms_of(N)
    slack = [2.0 * (math.log2(P) + 4.0) * 2.0 ** -53 * float(np.abs(fw['k'] * fw['a']).sum() / fw['Z']) * abs(g[n, 0])
             for n, fw in enumerate(want[3])]
    assert_grad(dm, want[2], 'tied', slack)


def test_alone_in_a_batch_again_on_a_stream_and_in_a_reused_workspace():
    mhw, hw = (14, 28), (120, 240)
    maps, G, fix = case(mhw, hw)
    g = gterms_of(N)
    base = run(maps, G, fix, gterms=g)
    again = run(maps, G, fix, gterms=g)
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(base, again))
    alone = run(maps[4:], G[4:], fix[4:], gterms=g[4:])
    assert all(np.array_equal(x, y[4:], equal_nan=True) for x, y in zip(alone, base))
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        other = run(maps, G, fix, gterms=g)
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(base, other))
    work = ops.sup_loss_work(2 * N, mhw, hw, torch.device(DEV, torch.cuda.current_device()))
    work.fill_(float('nan'))
    assert ops.sup_loss_work(N, mhw, hw, work.device, work) is work
    for _ in range(2):
        reused = run(maps, G, fix, gterms=g, work=work)
        assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(base, reused))


def test_a_workspace_that_is_too_small_is_refused():
    mhw, hw = (5, 9), (12, 24)
    maps, G, _ = case(mhw, hw)
    m, g, a = dev(maps), dev(G), wt(hw[0])
    L = _lib.lib()
    need = L.cp360_sup_loss_work_bytes(N, mhw[0], mhw[1], hw[0], hw[1])
    assert need == N * hw[0] * hw[1] * 12
    work = torch.empty(need // 8, dtype=torch.float64, device=DEV)
    terms = torch.full((N, 3), 7.0, dtype=torch.float64, device=DEV)
    valid = torch.zeros((N, 3), dtype=torch.uint8, device=DEV)
    stats = torch.zeros((N, 16), dtype=torch.float64, device=DEV)
    dm = torch.full_like(m, 7.0)
    p = ops.ptr
    assert L.cp360_sup_loss_forward(p(m), p(g), None, p(a), N, mhw[0], mhw[1], hw[0], hw[1], EPS, p(terms), p(valid), p(stats), p(work),
                                    need - 16, None) == -1
    assert L.cp360_sup_loss_backward(p(m), p(g), None, p(a), p(stats), p(valid), p(terms), N, mhw[0], mhw[1], hw[0], hw[1], EPS, p(dm),
                                     p(work), need - 16, None) == -1
    torch.cuda.synchronize()
    assert torch.all(terms == 7.0) and torch.all(dm == 7.0)            # nothing was launched
    short = torch.empty(4, dtype=torch.float64, device=DEV)            # the wrapper replaces it
    assert ops.sup_loss_work(N, mhw, hw, short.device, short).numel() * 8 >= need
    with pytest.raises(ValueError):
        ops.sup_loss_forward(m, g[:, :, :12].contiguous(), wt(7))
    with pytest.raises(ValueError):
        ops.sup_loss_backward(m, g, a, stats[:, :8].contiguous(), valid, terms)


# ----------------------------------------------------------------------------- the autograd function
def test_supervised_losses_means_counts_and_missing_gradients():
    """supervised_losses on [B, L] maps: the means over the valid maps and their counts; a term nobody differentiates sends no
    gradient; with no valid map every value is 0 and the gradient is exactly 0."""
    mhw, hw = (5, 9), (12, 24)
    maps, G, fix = case(mhw, hw)
    m4 = np.concatenate([maps, np.full((1,) + mhw, 0.5, np.float32)])[None]           # [1, 6, 5, 9]: the last map is flat
    g4, f4 = np.concatenate([G, G[:1]])[None], np.concatenate([fix, fix[:1]])[None]
    want = sr.backward(m4[0], g4[0], rs.weights(hw[0]), np.tile([0.2, 0.0, 0.0], (6, 1)), f4[0])
    assert want[1].sum(0).tolist() == [5, 5, 5]
    x = dev(m4).requires_grad_(True)
    kl, cc, nss, counts = ts.supervised_losses(x, dev(g4), dev(f4))
    assert counts.tolist() == [5, 5, 5] and counts.dtype == torch.int64 and kl.dtype == torch.float64
    for t, got in enumerate((kl, cc, nss)):
        assert abs(got.item() - want[0][:5, t].mean()) <= 1e-9 * max(1.0, abs(want[0][:5, t].mean()))
    kl.backward()                                                      # cc and nss get no gradient: None in backward
    assert_grad(x.grad[0].cpu().numpy(), want[2])
    flat = torch.full((2, 2, 5, 9), 0.25, device=DEV, requires_grad=True)
    kl, cc, nss, counts = ts.supervised_losses(flat, dev(g4)[:, :4].reshape(2, 2, *hw))
    assert counts.tolist() == [0, 0, 0] and (kl.item(), cc.item(), nss.item()) == (0.0, 0.0, 0.0)
    (kl - cc - nss).backward()
    assert torch.all(flat.grad == 0.0)
    with pytest.raises(ValueError):
        ts.supervised_losses(flat, dev(g4))


# ----------------------------------------------------------------------------- through the model
MODEL_EPS = 1e-6


def model_case(seed=1950):
    """ConvLSTMCell(8, 8), B = 2, T = 5, w = 7, the loss grid 30 x 60; the ground truth is a blob of 10 degrees that moves 6
    degrees a frame (``FixationMaps.density`` and ``.mask``), five fixations around its centre per frame."""
    B, T, C, w, hw = 2, 5, 8, 7, (30, 60)
    cell = ConvLSTMCell(C, C, precision='fp32')
    sd = synth.clstm_state(seed=seed, input_size=C, hidden_size=C)
    cell.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    cell.to(DEV)
    seq = torch.from_numpy(hashrng.uniform(seed + 1, (B, T, 6, C, w, w), 0.0, 1.0, dtype=np.float64).astype(np.float32)).to(DEV)
    lon = np.deg2rad(np.array([[6.0 * t + 90.0 * b - 30.0 for t in range(T)] for b in range(B)])).reshape(-1)
    lat = np.deg2rad(np.array([[10.0 - 25.0 * b for t in range(T)] for b in range(B)])).reshape(-1)
    off = np.deg2rad(3.0) * np.array([[0, 0], [1, 0], [-1, 0], [0, 1], [0, -1]], np.float64)
    lonlat = (np.stack([lon, lat], 1)[:, None, :] + off[None]).reshape(-1, 2)
    offsets = np.arange(B * T + 1, dtype=np.int32) * 5
    fm = fixations.FixationMaps(hw, sigma_deg=10.0, device=DEV)
    gt = fm.density(lonlat, offsets).reshape(B, T, *hw)
    fix = fm.mask(lonlat, offsets).reshape(B, T, *hw)
    return cell, seq, gt, fix


def test_parameter_gradients_match_the_torch_composition():
    """The window's parameter gradients with the loss in HIP against the same loss composed from torch on the same maps, within
    tests/test_train_gpu.py's bound for the small cell's gradients (1e-3 of the largest).  The torch side runs in float64 (its
    float32 KL cancels k at a tied minimum); kl_eps = 1e-6, a training value: at 2^-52 the slopes of the pixels tied on a clamped
    row reach Q / eps and the comparison would be of those alone."""
    cell, seq, gt, fix = model_case()
    B, T, _, C, w, _ = seq.shape
    frames = normalize_batch(seq).permute(0, 1, 2, 4, 5, 3).reshape(B, T, 6 * w * w, C).contiguous()
    grads = []
    for device_loss in (True, False):
        cell.zero_grad()
        maps = window_maps(cell, frames, range(T))
        if device_loss:
            kl, cc, nss, counts = ts.supervised_losses(maps, gt, fix, kl_eps=MODEL_EPS)
        else:
            kl, cc, nss, counts = ts.supervised_losses_torch(maps.double(), gt, fix, kl_eps=MODEL_EPS)
        assert counts.tolist() == [B * T] * 3
        (kl - cc - 0.1 * nss).backward()
        grads.append(({n: p.grad.detach().cpu().numpy().copy() for n, p in cell.named_parameters()},
                      [v.item() for v in (kl, cc, nss)]))
    (got, terms), (want, want_terms) = grads
    print('terms', terms, 'against', want_terms)
    assert np.allclose(terms, want_terms, rtol=1e-6, atol=1e-6)
    for n in want:
        err = float(np.max(np.abs(got[n] - want[n])) / max(np.max(np.abs(want[n])), 1e-30))
        print('%s: largest gradient %.3e, apart %.2e of it' % (n, np.max(np.abs(want[n])), err))
        assert np.max(np.abs(want[n])) > 0 and err <= 1e-3, n


# ----------------------------------------------------------------------------- end to end
TRAIN_ITERS = 30


@pytest.mark.parametrize('fused', [False, True])
def test_training_on_ground_truth_lowers_the_loss_and_raises_the_cc(fused):
    """One batch, TRAIN_ITERS iterations of train_step_gt with Adam (once with FusedAdam): the loss falls and the mean CC that
    SphereEval reports rises.  kl_eps is the metric's 2^-52 (cfg names none): the ground truth is about 1e-12 of its peak on
    the clamped rows, so the slopes Q / eps of the pixels tied there do not swamp the other terms (the largest parameter
    gradient of the first iterations is 0.12 .. 0.9 at 2^-52 and at 1e-6 alike).  Measured on the MI355X: DESIGN.md "K18"."""
    cell, seq, gt, fix = model_case(1960)
    cfg = types.SimpleNamespace(l_kl=1.0, l_cc=1.0, l_nss=0.1)
    opt = FusedAdam(cell, lr=2e-3) if fused else torch.optim.Adam(cell.parameters(), lr=2e-3)
    B, T, _, C, w, _ = seq.shape
    ev = eval_sphere.SphereEval((30, 60), device=DEV)

    def measure():
        with torch.no_grad():
            frames = normalize_batch(seq).permute(0, 1, 2, 4, 5, 3).reshape(B, T, 6 * w * w, C).contiguous()
            maps = window_maps(cell, frames, range(T))
            kl, cc, nss, _ = ts.supervised_losses(maps, gt, fix)
            means = ev.means(ev.evaluate(maps.reshape(B * T, *maps.shape[2:]), gt.reshape(B * T, 30, 60), fix.reshape(B * T, 30, 60)))
        return float(cfg.l_kl * kl - cfg.l_cc * cc - cfg.l_nss * nss), means['cc'], means['kl'], means['nss']

    before = measure()
    first = None
    for it in range(TRAIN_ITERS):
        kl, cc, nss, counts = ts.train_step_gt(cell, [seq[:, t] for t in range(T)], gt, opt, cfg, fix)
        if first is None:
            first = float(kl - cc - 0.1 * nss)
    assert counts.tolist() == [B * T] * 3 and counts.dtype == torch.int64
    after = measure()
    print('%s: loss %.6f -> %.6f; SphereEval cc %.6f -> %.6f, kl %.6f -> %.6f, nss %.6f -> %.6f' % (
        'FusedAdam' if fused else 'Adam', before[0], after[0], before[1], after[1], before[2], after[2], before[3], after[3]))
    assert abs(first - before[0]) <= 1e-9 * max(1.0, abs(before[0]))   # the step reports the loss it started from
    assert after[0] < before[0] and after[1] > before[1]
