"""Saliency metrics: CPU sanity of the oracle restatement, and the bf16
acceptance gate on the GPU - AUC-Judd and CC of the build's map vs a fixation map sampled from
the oracle's map must be within 1e-3 of the same metrics of the oracle's map, and
CC(build, oracle) >= 0.9999.  Below that: K8 (csrc/metrics.hip) at its edges - the resize bit for bit at
every kind of shape, the AUCs at the ends of n_fix, with ties, at every split count and step size, CC and SIM
against float64 numpy, and the refusal of maps whose normalisation is undefined."""
import numpy as np
import pytest
import torch

from oracle import o_metrics
from cp_360_weakly_supervised_saliency_amd.utils import synth, hashrng


def test_resize_linear_properties():
    a = hashrng.uniform(1, (14, 28))
    assert np.array_equal(o_metrics.resize_linear(a, (28, 14)), a)            # same size = identity
    up = o_metrics.resize_linear(a, (240, 120))
    assert up.shape == (120, 240) and up.min() >= a.min() - 1e-6 and up.max() <= a.max() + 1e-6
    const = o_metrics.resize_linear(np.full((960, 1920), 3.0, np.float32), (240, 120))
    assert np.all(const == 3.0)
    # 2x downscale of a ramp samples between pixel pairs: (x0 + x1)/2 at half-pixel centres
    ramp = np.tile(np.arange(8, dtype=np.float32), (2, 1))
    assert np.allclose(o_metrics.resize_linear(ramp, (4, 2))[0], [0.5, 2.5, 4.5, 6.5])


def test_metric_sanity():
    fix = synth.fixation_map(100, 240, 480, sigma=6.0)
    good = fix + 0.01 * hashrng.uniform(2, fix.shape)
    bad = hashrng.uniform(3, fix.shape)
    rng = np.random.RandomState(0)
    assert o_metrics.auc_judd(good, fix, rng=rng) > 0.95
    assert 0.3 < o_metrics.auc_judd(bad, fix, rng=np.random.RandomState(0)) < 0.7
    assert abs(o_metrics.corr_coeff(fix, fix) - 1.0) < 1e-6
    assert abs(o_metrics.corr_coeff(bad, fix)) < 0.1
    assert abs(o_metrics.similarity(fix, fix) - 1.0) < 1e-6
    assert o_metrics.auc_borji(good, fix, n_splits=5, rng=np.random.RandomState(0)) > 0.8
    with pytest.raises(ValueError):
        o_metrics.auc_judd(good, np.zeros_like(fix))


def test_oracle_metrics_match_reference_goldens(golden_dir):
    """tests/golden/metrics.npz holds AUC_Judd / CorrCoeff / similarity / AUC_Borji as computed by the
    reference's own utils/eval_saliency.py (make_golden.py: gen_metrics) on seeded maps; the oracle
    restatement must reproduce them (same resize, same RandomState(0) stream)."""
    import os
    from tests.golden.make_golden import METRIC_CASES, metric_inputs
    g = np.load(os.path.join(golden_dir, 'metrics.npz'))
    for k in range(len(METRIC_CASES)):
        sal, gt = metric_inputs(k)
        assert abs(o_metrics.auc_judd(sal, gt, rng=np.random.RandomState(0)) - float(g['auc_judd_%d' % k])) <= 1e-12
        assert abs(o_metrics.corr_coeff(sal, gt) - float(g['cc_%d' % k])) <= 1e-6
        assert abs(o_metrics.similarity(sal, gt) - float(g['sim_%d' % k])) <= 1e-7
        assert abs(o_metrics.auc_borji(sal, gt, n_splits=10, rng=np.random.RandomState(0))
                   - float(g['auc_borji_%d' % k])) <= 1e-12


@pytest.mark.gpu
def test_hip_auc_judd_without_jitter_normalises_in_float32(golden_dir):
    """AUC_Judd(jitter=False), utils/eval_saliency.py:104-116 without the float64 randn term: the float32 map is
    normalised in float32 (numpy type promotion) - HIP == the oracle, whose numpy arithmetic has exactly that typing,
    including maps with many exact ties (quantised values), where the last bit of the normalisation decides ranks."""
    from tests.golden.make_golden import METRIC_CASES, metric_inputs
    from cp_360_weakly_supervised_saliency_amd.utils import eval_saliency as ev
    for k in range(len(METRIC_CASES)):
        sal, gt = metric_inputs(k)
        for s in (sal, np.round(sal * 37.0).astype(np.float32) / np.float32(37.0) * np.float32(1.7)):
            want = o_metrics.auc_judd(s, gt, jitter=False)
            assert abs(ev.AUC_Judd(s, gt, jitter=False) - want) <= 1e-12, k


@pytest.mark.gpu
def test_hip_metrics_match_reference_goldens_and_oracle(golden_dir):
    """K8 (csrc/metrics.hip) behind the reference's names: the seeded cases of tests/golden/metrics.npz
    (values computed by the reference's own eval_saliency.py) and the oracle on a second set of maps."""
    import os
    from tests.golden.make_golden import METRIC_CASES, metric_inputs
    from cp_360_weakly_supervised_saliency_amd.utils import eval_saliency as ev
    g = np.load(os.path.join(golden_dir, 'metrics.npz'))
    for k in range(len(METRIC_CASES)):
        sal, gt = metric_inputs(k)
        np.random.seed(0)
        assert abs(ev.AUC_Judd(sal, gt) - float(g['auc_judd_%d' % k])) <= 1e-9
        assert abs(ev.CorrCoeff(sal, gt) - float(g['cc_%d' % k])) <= 2e-6
        assert abs(ev.similarity(sal, gt) - float(g['sim_%d' % k])) <= 2e-6
        np.random.seed(0)
        assert abs(ev.AUC_Borji(sal, gt, Nsplits=10) - float(g['auc_borji_%d' % k])) <= 1e-9
    # resize and metrics on device tensors, against the oracle
    a = hashrng.uniform(21, (14, 28))
    up = ev.resize_linear(torch.from_numpy(a).cuda()).cpu().numpy()
    assert np.array_equal(up, o_metrics.resize_linear(a, (240, 120)))
    fix = synth.fixations_from_map(a, 300, 480, 960)
    np.random.seed(5)
    got = ev.AUC_Judd(torch.from_numpy(a).cuda(), torch.from_numpy(fix).cuda())
    assert abs(got - o_metrics.auc_judd(a, fix, rng=np.random.RandomState(5))) <= 1e-9
    with pytest.raises(ValueError):
        ev.AUC_Judd(a, np.zeros_like(fix))


@pytest.mark.gpu
@pytest.mark.parametrize('T', [5, 16])
def test_bf16_auc_cc_gate_full_size(T):
    """T-frame 960x1920 clip (T = 5: the reference's seq_len; 16: the benchmark's), cube 224,
    full-size networks: oracle (fp32 CPU) vs the HIP path in fp32 and bf16.
    Gate (north star): |dAUC-Judd| <= 1e-3 and |dCC| <= 1e-3."""
    from cp_360_weakly_supervised_saliency_amd.pipeline import SaliencyEngine
    from tests.parity_helpers import oracle_pipeline
    H, W, cd = 960, 1920, 224
    rs = synth.resnet50_state(seed=1)
    cs = synth.clstm_state(seed=2)
    clip = synth.clip_u8(40, T, H, W)
    ref = oracle_pipeline(clip, rs, cs, cd)
    # fixations sampled from the oracle map: the oracle scores well above chance, so the 1e-3 gate discriminates
    fix = synth.fixations_from_map(ref, 140, H // 2, W // 2)
    frames = torch.from_numpy(clip[None]).cuda()

    def metrics(m):
        return (o_metrics.auc_judd(m, fix, rng=np.random.RandomState(0)), o_metrics.corr_coeff(m, fix))

    auc_ref, cc_ref = metrics(ref)
    out = {}
    for prec in ('fp32', 'bf16', 'fp16'):
        eng = SaliencyEngine(rs, cs, (H, W), cd, clips=1, frames=T, precision=prec)
        sal = eng(frames).cpu().numpy()[0]
        auc, cc = metrics(sal)
        out[prec] = (float(np.max(np.abs(sal - ref))), auc - auc_ref, cc - cc_ref,
                     o_metrics.corr_coeff(sal, ref))
        del eng
        torch.cuda.empty_cache()
    print('bf16/fp32 gate:', out, 'oracle AUC %.4f CC %.4f' % (auc_ref, cc_ref))
    assert auc_ref > 0.7 and cc_ref > 0.1
    assert out['fp32'][0] <= 1e-3
    assert min(out[p][3] for p in out) >= 0.9999, out          # CC(build, oracle)
    assert abs(out['fp32'][1]) <= 1e-3 and abs(out['fp32'][2]) <= 1e-3
    assert abs(out['bf16'][1]) <= 1e-3 and abs(out['bf16'][2]) <= 1e-3, out
    assert abs(out['fp16'][1]) <= 1e-3 and abs(out['fp16'][2]) <= 1e-3, out


# ======================================================================================================================
# K8 at its edges: every entry point of csrc/metrics.hip against the oracle (oracle/o_metrics.py) or float64 numpy written
# here, on maps from hashrng / synth.  The inputs are built once (lru_cache), and each builder asserts on the CPU what the
# expected value rests on; test_edge_inputs_hold_their_conditions runs those assertions without a GPU.
# ======================================================================================================================
import functools

GRID = (120, 240)                                   # the metrics' working size (height, width)


def _ev():
    from cp_360_weakly_supervised_saliency_amd.utils import eval_saliency as ev
    return ev


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(got, want):
    """float32 arrays, bit for bit (-0.0 is not 0.0); a NaN matches any NaN: its sign and payload are not specified by
    IEEE 754 for 0 * inf or inf - inf, and x86 and the GPU choose differently."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    ok = ~np.isnan(want)
    return torch.equal(torch.from_numpy(got.view(np.int32)[ok]), torch.from_numpy(want.view(np.int32)[ok]))


def count_above_two_sigma(F):
    """#{F > mean(F) + 2 std(F)} of a float32 map on the working grid, asserting that it is unambiguous: numpy evaluates the
    threshold with float32 pairwise sums, the kernel from float64 sums rounded once (metrics.hip's header: ~1e-7 relative apart)
    - no pixel may lie between the two float32 thresholds.  A condition on the inputs, not a tolerance."""
    assert F.dtype == np.float32 and F.shape == GRID
    t_numpy = np.mean(F) + 2 * np.std(F)
    assert t_numpy.dtype == np.float32
    F64 = F.astype(np.float64)
    t_kernel = np.float32(F64.mean() + 2.0 * np.sqrt(np.mean((F64 - F64.mean()) ** 2)))
    lo, hi = min(t_numpy, t_kernel), max(t_numpy, t_kernel)
    assert abs(float(hi) - float(lo)) <= 4e-7 * abs(float(hi)), (t_numpy, t_kernel)
    assert not np.any((F > lo) & (F <= hi)), (t_numpy, t_kernel)
    return int(np.count_nonzero(F > t_numpy))


def fixation_count(gt):
    """n_fix of a float32 fixation map (resized first, as every metric does)."""
    gt = np.asarray(gt)
    assert gt.dtype == np.float32
    return count_above_two_sigma(o_metrics.resize_linear(gt, GRID[::-1]))


def binary_map(seed, p, shape=GRID):
    return (hashrng.uniform(seed, shape) < p).astype(np.float32)


# ----------------------------------------------------------------------------- resize
RESIZE_PAIRS = [((960, 1920), (120, 240)), ((512, 1024), (120, 240)), ((100, 200), (120, 240)), ((37, 53), (120, 240)),
                ((1, 1), (5, 7)), ((1, 9), (4, 3)), ((9, 1), (3, 4)), ((120, 240), (120, 240)), ((14, 28), (33, 66))]


@pytest.mark.gpu
@pytest.mark.parametrize('src,dst', RESIZE_PAIRS)
def test_hip_resize_bit_for_bit(src, dst):
    """8x down (every fraction 0.5), non-integer down, 1.2x up, anisotropic odd sizes, both clamps at once with fewer than 256
    outputs, a single source row, a single source column, the identity, and 2178 outputs (no multiple of 256)."""
    ev = _ev()
    a = hashrng.uniform(8900 + src[0], src, -1.0, 3.0)
    want = o_metrics.resize_linear(a, (dst[1], dst[0]))
    assert want.dtype == np.float32 and want.shape == dst
    from_numpy = ev.resize_linear(a, dsize=(dst[1], dst[0]))
    from_tensor = ev.resize_linear(_cuda(a), dsize=(dst[1], dst[0]))
    assert from_numpy.dtype == torch.float32 and tuple(from_numpy.shape) == dst
    assert torch.equal(from_numpy.view(torch.int32), from_tensor.view(torch.int32))
    assert torch.equal(from_numpy.cpu().view(torch.int32), torch.from_numpy(want).view(torch.int32))


def special_source():
    a = hashrng.uniform(8950, (6, 9), 0.5, 2.0)
    a[0, 0], a[1, 4], a[3, 2], a[4, 7], a[5, 8] = -0.0, np.inf, -np.inf, np.nan, 1e-41
    with np.errstate(invalid='ignore'):
        want = o_metrics.resize_linear(a, (31, 17))
    return a, want


@pytest.mark.gpu
def test_hip_resize_special_values():
    """-0.0, inf, -inf, nan and a subnormal in known pixels of a 6 x 9 map, resized to 17 x 31: the non-finite outputs are the
    oracle's (the taps that reach the pixel, 0 * inf = NaN included), everything else bit for bit."""
    ev = _ev()
    a, want = special_source()
    got = ev.resize_linear(a, dsize=(31, 17)).cpu().numpy()
    assert np.array_equal(np.isposinf(got), np.isposinf(want)) and np.array_equal(np.isneginf(got), np.isneginf(want))
    assert same_bits(got, want)
    assert same_bits(ev.resize_linear(_cuda(a), dsize=(31, 17)).cpu().numpy(), want)


# ----------------------------------------------------------------------------- AUC_Judd
@functools.lru_cache(maxsize=None)
def judd_case(name):
    """(saliency f32, fixation map f32, n_fix, the oracle's AUC_Judd(jitter=False))."""
    sal = hashrng.uniform(9000, GRID) ** 2
    if name == 'one_fixation':
        gt = np.zeros(GRID, np.float32)
        gt[37, 101] = 1.0
        want_fix = 1
    elif name == 'ceiling':                         # F > mean + 2 std selects at most a fifth of the pixels (Cantelli)
        gt, want_fix = binary_map(5, 0.19), 5419
    elif name == 'none':                            # >= 20 % ones: no pixel passes
        gt, want_fix = binary_map(5, 0.25), 0
    elif name == 'eight_levels':
        sal = (np.floor(hashrng.uniform(9001, GRID) * 8.0) / 8.0).astype(np.float32)
        gt, want_fix = binary_map(9002, 0.04), None
    elif name == 'resized':                         # both maps go through the resize; the fixation map is no longer binary
        sal = hashrng.uniform(9003, (32, 64)) ** 2
        gt, want_fix = binary_map(9004, 0.04, (480, 960)), None
    n_fix = fixation_count(gt)
    assert want_fix is None or n_fix == want_fix, n_fix
    if name == 'eight_levels':                      # ties inside the fixated set, outside it and across it
        fixed = gt > 0
        for level in np.unique(sal):
            assert np.count_nonzero(fixed & (sal == level)) >= 2 and np.count_nonzero(~fixed & (sal == level)) >= 2
        assert len(np.unique(sal)) == 8
    return sal.astype(np.float32), gt, n_fix, o_metrics.auc_judd(sal.astype(np.float32), gt, jitter=False)


JUDD_CASES = ['one_fixation', 'ceiling', 'none', 'eight_levels', 'resized']


@pytest.mark.gpu
@pytest.mark.parametrize('name', JUDD_CASES)
def test_hip_auc_judd_edges(name):
    """jitter=False against the oracle, <= 1e-12: at most 5421 float64 terms that sum to at most 1 (n eps ~ 6e-13)."""
    sal, gt, n_fix, want = judd_case(name)
    got = _ev().AUC_Judd(sal, gt, jitter=False)
    print('AUC_Judd %s: n_fix %d, hip %.17g, oracle %.17g, gap %.3e' % (name, n_fix, got, want, abs(got - want)))
    assert abs(got - want) <= 1e-12
    if name == 'none':
        assert got == 0.5 and want == 0.5


@pytest.mark.gpu
@pytest.mark.parametrize('seed', [0, 7])
def test_hip_auc_judd_jitter_input_types(seed):
    """The same map as a float64 ndarray, a float32 ndarray and a float32 device tensor, np.random.seed(s) before each call: the
    three results are the same bits, and each is the oracle's with RandomState(s) (<= 1e-9, as the golden test)."""
    ev = _ev()
    sal, gt, _, _ = judd_case('resized')
    want = o_metrics.auc_judd(sal, gt, rng=np.random.RandomState(seed))
    got = []
    for s, g in ((sal.astype(np.float64), gt.astype(np.float64)), (sal, gt), (_cuda(sal), _cuda(gt))):
        np.random.seed(seed)
        got.append(ev.AUC_Judd(s, g))
    print('AUC_Judd jitter seed %d: hip %.17g, oracle %.17g, gap %.3e' % (seed, got[0], want, abs(got[0] - want)))
    assert got[0] == got[1] == got[2]
    assert abs(got[0] - want) <= 1e-9


# ----------------------------------------------------------------------------- AUC_Borji
@functools.lru_cache(maxsize=None)
def borji_case(name):
    """(saliency f32, fixation map f32, n_fix)."""
    if name == 'lattice':                           # round(100 s) / 100 in float32, 0 and 1 included: the normalisation is exact
        sal = (np.round(hashrng.uniform(9100, GRID) * 100.0) / np.float32(100.0)).astype(np.float32)
        assert sal.min() == 0.0 and sal.max() == 1.0 and len(np.unique(sal)) == 101
    elif name == 'clipped':                         # a long tail: S[S > mean + 2 std] = 1 changes pixels
        sal = (hashrng.uniform(9101, (60, 120)) ** 6).astype(np.float32)
    else:
        sal = (hashrng.uniform(9102, (32, 64)) ** 2).astype(np.float32)
    S = o_metrics.resize_linear(sal, GRID[::-1])
    changed = count_above_two_sigma(S)              # the S[S > mean + 2 std] = 1 step (:37-38), unambiguous as well
    if name == 'lattice':
        assert changed == 0                         # ... so S stays on the lattice
        norm = (S - np.min(S)) / (np.max(S) - np.min(S))
        assert norm.dtype == np.float32 and np.array_equal(norm, sal)
    if name == 'clipped':
        assert changed > 100 and np.max(S) < 1.0    # the step writes a value the map did not hold
    if name == 'plain':                             # fixations that follow the map, as in the goldens
        gt = synth.fixations_from_map(sal, 9110, 480, 960).astype(np.float32)
    else:                                           # ... and a 480 x 960 binary map, no longer binary after its resize
        gt = binary_map(9111, 0.04, (480, 960))
    n_fix = fixation_count(gt)
    assert n_fix > (30 if name == 'plain' else 1000)
    return sal, gt, n_fix


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['plain', 'lattice', 'clipped'])
def test_hip_auc_borji_splits_and_steps(name):
    """Nsplits 1, 10 and the default 100, stepSize 0.01, 0.05, 0.013 (does not divide 1) and 0.25 (4 thresholds), against the
    oracle with RandomState(s), <= 1e-12: a split is a sum of at most 102 products of exact count ratios, the result a mean.

    'lattice': S = round(100 s) / 100 in float32, and every threshold k stepSize is a float64.  The kernel compares
    (double)S >= t, which is numpy 2's promotion of a float32 array against an np.float64 scalar (np.arange yields those;
    numpy 2.2.6 produced the oracle's values here): float32(0.29) < 0.29 in float64 but float32(0.3) > 0.3, so a float32
    comparison, or numpy 1's value-based casting of the scalar, would count differently."""
    ev = _ev()
    sal, gt, n_fix = borji_case(name)
    worst = 0.0
    for n_splits in (1, 10, 100):
        for step in (0.01, 0.05, 0.013, 0.25):
            seed = 100 * n_splits + int(step * 1000)
            want = o_metrics.auc_borji(sal, gt, n_splits=n_splits, step=step, rng=np.random.RandomState(seed))
            np.random.seed(seed)
            got = ev.AUC_Borji(sal, gt, Nsplits=n_splits, stepSize=step)
            worst = max(worst, abs(got - want))
            assert abs(got - want) <= 1e-12, (n_splits, step, got, want)
    np.random.seed(3)
    default = ev.AUC_Borji(sal, gt)                                      # Nsplits=100, stepSize=0.01
    assert abs(default - o_metrics.auc_borji(sal, gt, rng=np.random.RandomState(3))) <= 1e-12
    print('AUC_Borji %s: n_fix %d, largest gap over 12 settings %.3e' % (name, n_fix, worst))
    with pytest.raises(ValueError):
        ev.AUC_Borji(sal, gt, Nsplits=10, stepSize=0.005)                # the table holds at most 102 thresholds


# ----------------------------------------------------------------------------- CC and SIM
def cc_sim_float64(a32, b32):
    """eval_saliency.py:149-190 in float64 numpy on the (already resized) float32 maps."""
    a, b = a32.astype(np.float64), b32.astype(np.float64)
    za, zb = (a - a.mean()) / a.std(), (b - b.mean()) / b.std()
    da, db = za - za.mean(), zb - zb.mean()
    cc = np.sum(da * db) / np.sqrt(np.sum(da ** 2) * np.sum(db ** 2))
    na, nb = (a - a.min()) / (a.max() - a.min()), (b - b.min()) / (b.max() - b.min())
    return float(cc), float(np.sum(np.minimum(na / na.sum(), nb / nb.sum())))


@functools.lru_cache(maxsize=None)
def cc_sim_case(name):
    """(map1 f32, map2 f32, float64 CC, float64 SIM)."""
    shape = {'14x28': (14, 28), '120x240': GRID, 'anti': GRID, '480x960': (480, 960)}[name]
    a = hashrng.uniform(9200 + shape[0], shape) ** 2
    noise = hashrng.uniform(9300 + shape[0], shape)
    b = (1.0 - a + 0.5 * noise) if name == 'anti' else (a + 0.5 * noise)
    a, b = a.astype(np.float32), b.astype(np.float32)
    ra, rb = o_metrics.resize_linear(a, GRID[::-1]), o_metrics.resize_linear(b, GRID[::-1])
    assert ra.dtype == np.float32 and rb.dtype == np.float32
    cc, sim = cc_sim_float64(ra, rb)
    if shape == GRID:                               # the oracle's resize is the identity there: feed it the float64 casts
        assert np.array_equal(ra, a) and np.array_equal(rb, b)
        assert abs(o_metrics.corr_coeff(ra.astype(np.float64), rb.astype(np.float64)) - cc) <= 1e-12
        assert abs(o_metrics.similarity(ra.astype(np.float64), rb.astype(np.float64)) - sim) <= 1e-12
    assert (cc < -0.5) if name == 'anti' else (cc > 0.5)
    return a, b, cc, sim


CC_SIM_CASES = ['14x28', '120x240', 'anti', '480x960']


@pytest.mark.gpu
@pytest.mark.parametrize('name', CC_SIM_CASES)
def test_hip_cc_sim_against_float64(name):
    """<= 1e-10 absolute: 28800 float64 terms give n eps ~ 3e-12, a 30-fold margin."""
    ev = _ev()
    a, b, cc, sim = cc_sim_case(name)
    got_cc, got_sim = ev.CorrCoeff(a, b), ev.similarity(_cuda(a), _cuda(b))
    print('%s: CC %.15f gap %.3e, SIM %.15f gap %.3e' % (name, got_cc, abs(got_cc - cc), got_sim, abs(got_sim - sim)))
    assert abs(got_cc - cc) <= 1e-10 and abs(got_sim - sim) <= 1e-10


@pytest.mark.gpu
def test_hip_cc_sim_of_a_flat_map_are_nan():
    ev = _ev()
    a, flat = cc_sim_case('120x240')[0], np.full(GRID, 0.25, np.float32)
    with np.errstate(invalid='ignore', divide='ignore'):
        assert np.isnan(cc_sim_float64(flat, a)).all() and np.isnan(cc_sim_float64(a, flat)).all()      # as numpy does
    for x, y in ((flat, a), (a, flat), (flat, flat)):
        assert np.isnan(ev.CorrCoeff(x, y)) and np.isnan(ev.similarity(x, y))


# ----------------------------------------------------------------------------- refusals
def undefined_maps():
    base = judd_case('one_fixation')[0]
    one_nan, one_inf = base.copy(), base.copy()
    one_nan[60, 7], one_inf[3, 200] = np.nan, np.inf
    return {'flat': np.full(GRID, 0.5, np.float32), 'nan': one_nan, 'inf': one_inf}


@pytest.mark.gpu
def test_hip_auc_refuses_undefined_normalisation():
    """A flat map (max == min: 0 / 0 everywhere), a map with one nan, a map with one inf: the reference prints 'NaN saliency_map'
    and exits; AUC_Judd and AUC_Borji raise ValueError with that text, and the next normal call returns the bits it returned
    before: the refusal leaves nothing behind.  A fixation map with >= 20 % ones has no pixel above mean + 2 std: AUC_Borji
    raises, AUC_Judd returns 0.5 (test_hip_auc_judd_edges['none']).  A flat finite map stays legal with the default jitter."""
    ev = _ev()
    sal, gt, _, _ = judd_case('ceiling')

    def normal_calls():
        np.random.seed(11)
        return (ev.AUC_Judd(sal, gt, jitter=False), ev.AUC_Judd(sal, gt), ev.AUC_Borji(sal, gt, Nsplits=10))

    before = normal_calls()
    assert all(np.isfinite(before))
    for name, bad in undefined_maps().items():
        with pytest.raises(ValueError, match='NaN saliency_map'):
            ev.AUC_Judd(bad, gt, jitter=False)
        assert normal_calls() == before, name
        with pytest.raises(ValueError, match='NaN saliency_map'):
            ev.AUC_Borji(bad, gt, Nsplits=10)
        assert normal_calls() == before, name
        if name != 'flat':
            with pytest.raises(ValueError, match='NaN saliency_map'):
                ev.AUC_Judd(bad, gt)
            with pytest.raises(ValueError, match='NaN saliency_map'):
                ev.AUC_Judd(_cuda(bad), _cuda(gt))
            assert normal_calls() == before, name
    none = judd_case('none')[1]
    with pytest.raises(ValueError):
        ev.AUC_Borji(sal, none, Nsplits=10)
    assert normal_calls() == before
    flat = undefined_maps()['flat']
    np.random.seed(4)
    got = ev.AUC_Judd(flat, gt)                                           # the jitter breaks the ties
    assert abs(got - o_metrics.auc_judd(flat, gt, rng=np.random.RandomState(4))) <= 1e-9


@pytest.mark.gpu
def test_c_entries_answer_nan_on_their_own():
    """The C ABI without the Python wrapper's checks: with the status that cp360_metric_auc_prepare records in the workspace,
    cp360_metric_auc_judd and cp360_metric_auc_borji write NaN; so does the latter when no pixel is fixated."""
    import ctypes as C
    from cp_360_weakly_supervised_saliency_amd._lib import check, lib, ptr, stream
    n = GRID[0] * GRID[1]
    gt = _cuda(judd_case('ceiling')[1])
    rr = torch.zeros((5419, 3), dtype=torch.int32, device='cuda')

    def run(sal, fix, mode):
        work = torch.empty(lib().cp360_metric_work_bytes(n), dtype=torch.uint8, device='cuda')
        check(lib().cp360_metric_auc_prepare(ptr(sal), ptr(fix), None, n, mode, ptr(work), stream()))
        head = work[:16].view(torch.float64).tolist()
        if mode == 0:
            out = torch.zeros(2, dtype=torch.float64, device='cuda')
            check(lib().cp360_metric_auc_judd(n, ptr(work), ptr(out), stream()))
            return head, out[:1].cpu().numpy()
        out = torch.zeros(3, dtype=torch.float64, device='cuda')
        check(lib().cp360_metric_auc_borji(n, 3, ptr(rr), C.c_double(0.01), ptr(work), ptr(out), stream()))
        return head, out.cpu().numpy()

    for name, bad in undefined_maps().items():
        for mode in (0, 1):
            head, out = run(_cuda(bad), gt, mode)
            assert head == [5419.0, 1.0] and np.isnan(out).all(), (name, mode)
    head, out = run(_cuda(judd_case('none')[0]), _cuda(judd_case('none')[1]), 1)
    assert head == [0.0, 0.0] and np.isnan(out).all()
    head, out = run(_cuda(judd_case('ceiling')[0]), gt, 0)
    assert head == [5419.0, 0.0] and abs(out[0] - judd_case('ceiling')[3]) <= 1e-12


# ----------------------------------------------------------------------------- the conditions, without a GPU
def test_edge_inputs_hold_their_conditions():
    """Everything the GPU tests above rest on that the CPU can check: the n_fix values (1, 5419, 0), no pixel between the two
    float32 fixation thresholds in any fixation map, the oracle's 0.5 for n_fix = 0, the lattice and clipping conditions of the
    AUC_Borji maps, the sign of the anticorrelated CC, and numpy's NaN for flat maps."""
    for name in JUDD_CASES:
        sal, gt, n_fix, want = judd_case(name)
        assert sal.dtype == np.float32 and gt.dtype == np.float32 and 0.0 <= want <= 1.0
    assert judd_case('none')[3] == 0.5 and judd_case('none')[2] == 0
    for name in ('plain', 'lattice', 'clipped'):
        borji_case(name)
    for name in CC_SIM_CASES:
        cc_sim_case(name)
    a, want = special_source()
    assert 0 < np.count_nonzero(~np.isfinite(want)) < want.size and np.isposinf(want).any() and np.isneginf(want).any()
    assert want[0, 0] == 0.0 and not np.signbit(want[0, 0])              # -0.0 * 1 + b * 0 = +0.0 at the clamped corner
    for bad in undefined_maps().values():
        with np.errstate(invalid='ignore'):
            S = (bad - np.min(bad)) / (np.max(bad) - np.min(bad))
        assert np.isnan(S).any()
