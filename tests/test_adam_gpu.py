"""The fused Adam step on the GPU (csrc/adam.hip, ops.adam_step / ops.adam_step_conv, train_temporal.FusedAdam): one step
against Adam in float64, the packs it writes against the packers byte for byte, and the optimizer inside train_step - the
packs stay current (no pack kernel runs in the next iteration), every other holder of packed weights still repacks, and the
trajectory follows torch.optim.Adam's.

The single-step bounds count roundings (at most 8 f32 operations on the update, one on the final subtraction), doubled:
|m - m64| <= 2^-22 |m64|, |v - v64| <= 2^-22 |v64|, |p - p64| <= 2^-23 |p64| + 2^-20 |d64| (d64: the float64 update).  They are
bounds of a well-conditioned update, so the inputs keep every sum free of cancellation: p, g and m of one element share a
sign (signs and magnitudes differ between elements).

The bounds count the roundings of operations, not the representation of constants, so the single-step tests run betas that are
exact in f32, (0.875, 1 - 2^-10): the float64 reference and the f32 code then run the same Adam, and a product with 1 - beta is
exact.  With torch's defaults (0.9, 0.999) the constant 1 - beta2 alone is 0.8 x 2^-24 away from its float64 value, and with
weight_decay = 0.01 - where g' = g + wd p is rounded before it is squared - torch.optim.Adam on the CPU itself then reaches
1.16 x the bound on exp_avg_sq (667 of 4.2 M elements).  With exact betas the worst case of the kernel is 1.37 (g', one fused
multiply-add, wd rounded to f32) x 2 (squared) + 1 (the final fused multiply-add) = 3.74 roundings of 2^-24 on exp_avg_sq and
3.37 on exp_avg, inside 2^-22.  The optimizer-level test below runs the defaults (weight_decay 0) against the same bounds."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from cp_360_weakly_supervised_saliency_amd import _lib, ops
from cp_360_weakly_supervised_saliency_amd.model.clstm import ConvLSTMCell
from cp_360_weakly_supervised_saliency_amd.model.clstm_train import trainer_of
from cp_360_weakly_supervised_saliency_amd.temporal_model import train_temporal as tt
from cp_360_weakly_supervised_saliency_amd.utils import hashrng, synth

pytestmark = pytest.mark.gpu
DEV = 'cuda'
HYPER = dict(lr=1e-3, betas=(0.875, 1 - 2.0 ** -10), eps=1e-8)      # betas exact in f32: see the module docstring
GRID_CAP = 4096 * 256 * 4          # elements one pass of the capped grid covers (adam_flat_kernel: 4096 x 256 x 16 bytes)


# ----------------------------------------------------------------------------- float64 reference and inputs
def adam64(p, g, m, v, lr, betas, eps, weight_decay, step):
    """Adam in float64 on f32 inputs -> (p, m, v, update)."""
    p, g, m, v = (a.astype(np.float64) for a in (p, g, m, v))
    b1, b2 = betas
    g = g + weight_decay * p
    m = m + (1 - b1) * (g - m)
    v = b2 * v + (1 - b2) * g * g
    d = (lr / (1 - b1 ** step)) * m / (np.sqrt(v) / np.sqrt(1 - b2 ** step) + eps)
    return p - d, m, v, d


def make_inputs(shape, seed, step):
    """p, g, m, v f32: magnitudes over seven decades, exact zeros in g; one sign per element.  Step 1 starts from m = v = 0
    (a zero gradient there leaves v = 0: the denominator is eps); later steps carry moments, zero where the gradient is."""
    rng = np.random.default_rng(seed)
    sign = np.where(rng.random(shape) < 0.5, -1.0, 1.0)
    mag = lambda: 10.0 ** rng.uniform(-6, 1, shape)
    g = sign * mag()
    zero = rng.random(shape) < 0.125
    g[zero] = 0.0
    p = sign * 10.0 ** rng.uniform(-4, 0, shape)
    if step == 1:
        m, v = np.zeros(shape), np.zeros(shape)
    else:
        m, v = sign * mag(), mag() ** 2
        dead = zero & (rng.random(shape) < 0.5)               # never saw a gradient: m = v = 0, the denominator is eps
        m[dead], v[dead] = 0.0, 0.0
    return tuple(a.astype(np.float32) for a in (p, g, m, v))


def assert_step(got, want, what):
    """The single-step bound of the module docstring; got = (p, m, v) f32, want = adam64's result."""
    p64, m64, v64, d64 = want
    p, m, v = (a.astype(np.float64) for a in got)
    em, ev = np.abs(m - m64) - 2.0 ** -22 * np.abs(m64), np.abs(v - v64) - 2.0 ** -22 * np.abs(v64)
    ep = np.abs(p - p64) - (2.0 ** -23 * np.abs(p64) + 2.0 ** -20 * np.abs(d64))
    print('%s: worst m %.3g ulp22, v %.3g ulp22, p %.3g of its bound' % (
        what, np.max(np.abs(m - m64) / np.maximum(2.0 ** -22 * np.abs(m64), 1e-300)),
        np.max(np.abs(v - v64) / np.maximum(2.0 ** -22 * np.abs(v64), 1e-300)),
        np.max(np.abs(p - p64) / np.maximum(2.0 ** -23 * np.abs(p64) + 2.0 ** -20 * np.abs(d64), 1e-300))))
    assert em.max() <= 0, (what, 'exp_avg', int(np.argmax(em)))
    assert ev.max() <= 0, (what, 'exp_avg_sq', int(np.argmax(ev)))
    assert ep.max() <= 0, (what, 'param', int(np.argmax(ep)))


def torch_cpu_step(p, g, m, v, weight_decay, step):
    """The same step with torch.optim.Adam on the CPU."""
    w = torch.nn.Parameter(torch.from_numpy(p.copy()))
    opt = torch.optim.Adam([w], weight_decay=weight_decay, foreach=False, **HYPER)
    w.grad = torch.from_numpy(g.copy())
    opt.state[w] = dict(step=torch.tensor(float(step - 1)), exp_avg=torch.from_numpy(m.copy()),
                        exp_avg_sq=torch.from_numpy(v.copy()))
    opt.step()
    return w.detach().numpy(), opt.state[w]['exp_avg'].numpy(), opt.state[w]['exp_avg_sq'].numpy()


def dev(*arrays):
    return tuple(torch.from_numpy(a.copy()).to(DEV) for a in arrays)


def host(*tensors):
    return tuple(t.cpu().numpy() for t in tensors)


# ----------------------------------------------------------------------------- single step
@pytest.mark.parametrize('step', [1, 1000])
@pytest.mark.parametrize('weight_decay', [0.0, 0.01])
@pytest.mark.parametrize('n', [1, 3, 4, 1023, 1025, GRID_CAP + 5])
def test_flat_step_against_float64(n, weight_decay, step):
    p, g, m, v = make_inputs((n,), 100 + n % 97 + step, step)
    want = adam64(p, g, m, v, weight_decay=weight_decay, step=step, **HYPER)
    tp, tg, tm, tv = dev(p, g, m, v)
    ops.adam_step(tp, tg, tm, tv, weight_decay=weight_decay, step=step, **HYPER)
    assert_step(host(tp, tm, tv), want, 'adam_step')
    assert_step(torch_cpu_step(p, g, m, v, weight_decay, step), want, 'torch CPU')       # the bound is not vacuous
    assert np.array_equal(tg.cpu().numpy(), g)                                           # the gradient is read only
    if step == 1 and weight_decay == 0 and n >= 1023:
        dead = g == 0                                                                    # v = 0: 0 / eps, no movement
        assert dead.any() and np.array_equal(tv.cpu().numpy()[dead], np.zeros(int(dead.sum()), np.float32))
        assert np.array_equal(tp.cpu().numpy()[dead], p[dead])


@pytest.mark.parametrize('step', [1, 1000])
@pytest.mark.parametrize('n', [1025, GRID_CAP + 5])
def test_flat_step_with_default_betas(n, step):
    """The constants users run, (0.9, 0.999), without weight decay: the rounded 1 - beta2 costs 0.8 of the 4 roundings the bound
    on exp_avg_sq allows, the two products and the sum at most 3 more only when they all err one way (see the module docstring)."""
    hyper = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    p, g, m, v = make_inputs((n,), 500 + step, step)
    want = adam64(p, g, m, v, weight_decay=0.0, step=step, **hyper)
    tp, tg, tm, tv = dev(p, g, m, v)
    ops.adam_step(tp, tg, tm, tv, step=step, **hyper)
    assert_step(host(tp, tm, tv), want, 'adam_step, default betas')


def test_division_and_square_root_are_correctly_rounded():
    """p, m, v bit for bit against the step in numpy float32, whose square root and division are correctly rounded.  With
    g = 0, p = 0, eps = 0 and the exact betas every other operation is a single rounding numpy restates exactly (m' = 0.875 m,
    v' = beta2 v, p' = -(lr / bc1) * (m' / (sqrt(v') / sqrt(bc2)))), so one ulp in the square root of any of the 2^18 values of v -
    a native, approximate v_sqrt_f32 is off on a large part of them - changes the bits of p."""
    n, step = 1 << 18, 10
    rng = np.random.default_rng(77)
    m = (np.where(rng.random(n) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-3, 1, n)).astype(np.float32)
    v = (10.0 ** rng.uniform(-8, 2, n)).astype(np.float32)
    z = np.zeros(n, np.float32)
    b1, b2 = HYPER['betas']
    f = np.float32
    m1 = (f(b1) * m).astype(np.float32)                                           # fma(0.125, 0 - m, m): one rounding of 0.875 m
    v1 = (f(b2) * v).astype(np.float32)
    denom = (np.sqrt(v1) / f(np.sqrt(1 - b2 ** step))).astype(np.float32)
    p1 = -(f(HYPER['lr'] / (1 - b1 ** step)) * (m1 / denom).astype(np.float32)).astype(np.float32)
    assert denom.dtype == np.float32 and p1.dtype == np.float32
    tp, tg, tm, tv = dev(z, z, m, v)
    ops.adam_step(tp, tg, tm, tv, lr=HYPER['lr'], betas=HYPER['betas'], eps=0.0, step=step)
    gp, gm, gv = host(tp, tm, tv)
    assert np.array_equal(gm, m1) and np.array_equal(gv, v1)
    print('square root pin: %d of %d parameters differ' % (int(np.sum(gp != p1)), n))
    assert np.array_equal(gp, p1)


def test_flat_step_is_reproducible_and_checks_arguments():
    p, g, m, v = make_inputs((70001,), 7, 1000)
    a, b = dev(p, g, m, v), dev(p, g, m, v)
    ops.adam_step(*a, step=1000, **HYPER)
    ops.adam_step(*b, step=1000, **HYPER)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    with pytest.raises(ValueError):
        ops.adam_step(a[0], a[1][:-1], a[2], a[3], step=1)                               # shapes
    with pytest.raises(ValueError):
        ops.adam_step(a[0], a[1].double(), a[2], a[3], step=1)                           # dtype
    with pytest.raises(ValueError):
        ops.adam_step(a[0][::2], a[1][::2], a[2][::2], a[3][::2], step=1)                # contiguity
    with pytest.raises(ValueError):
        ops.adam_step(*a, step=0)
    with pytest.raises(RuntimeError):
        ops.adam_step(a[0].cpu(), a[1], a[2], a[3], step=1)


# ----------------------------------------------------------------------------- the packs
FILTERS = [(32, 16, 8, 8), (256, 128, 64, 64), (288, 144, 0, 144), (40, 24, 8, 12)]      # c_out, c_in, dgrad ci0, n


def make_packs(w, dtype, ci0, n):
    """{'tap' / 'chan' / 'dgrad': uint8 pack} of filter w by the packers (a layout the library has no kernel for: absent)."""
    L = _lib.lib()
    conv = ops.Conv(w, None, None, 1, 1, True, dtype, w.device)
    packs = {}
    for name, d in (('tap', conv._desc(6, 8, 8, 1)), ('chan', conv._desc(6, 7, 7, 1, clip_resident=1))):
        nbytes = L.cp360_conv_packed_bytes(C.byref(d))
        if nbytes == 0:
            continue
        t = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
        _lib.check(L.cp360_conv_pack_weights(C.byref(d), _lib.ptr(w), None, _lib.ptr(t), 0, _lib.stream()))
        packs[name] = t
    packs['dgrad'] = ops.DgradPack(w, ci0, n, dtype).packed
    return packs


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('c_out,c_in,ci0,n', FILTERS)
def test_conv_step_writes_the_packers_bytes(c_out, c_in, ci0, n, dtype):
    shape = (c_out, c_in, 3, 3)
    p, g, m, v = make_inputs(shape, 300 + c_out, 1000)
    tp, tg, tm, tv = dev(p, g, m, v)
    packs = make_packs(tp, dtype, ci0, n)                      # of the OLD weights: every weight's bytes must change hands
    skipped = {'tap', 'chan', 'dgrad'} - set(packs)
    assert skipped <= ({'chan'} if c_out < 256 else set()), skipped
    old = {k: t.clone() for k, t in packs.items()}
    ops.adam_step_conv(tp, tg, tm, tv, weight_decay=0.01, step=1000, dtype=dtype, fwd_tap_major=packs['tap'],
                       fwd_chan_major=packs.get('chan'), dgrad_packed=packs['dgrad'], ci0=ci0, n_dgrad=n, **HYPER)
    fresh = make_packs(tp, dtype, ci0, n)                      # the packers on the kernel's own new p
    # a filter whose every byte is non-zero in both dtypes (0x3F8F0F0F): its packs have zero bytes exactly at the padding
    full = torch.full_like(tp, float(np.array(0x3F8F0F0F, np.uint32).view(np.float32)))
    pads = make_packs(full, dtype, ci0, n)
    for k in packs:
        assert not torch.equal(packs[k], old[k]), k
        assert torch.equal(packs[k], fresh[k]), k
        assert int(packs[k][pads[k] == 0].max() if (pads[k] == 0).any() else 0) == 0, k
    es = packs['dgrad'].numel() // (n * 9 * c_out)
    assert bool((pads['tap'] == 0).any()) == (c_out % 256 != 0 or c_in % (128 // es) != 0)

    # without packs: the same p, m, v bit for bit
    up, ug, um, uv = dev(p, g, m, v)
    ops.adam_step_conv(up, ug, um, uv, weight_decay=0.01, step=1000, dtype=dtype, **HYPER)
    assert torch.equal(up, tp) and torch.equal(um, tm) and torch.equal(uv, tv)
    # one pack at a time, the other pointers NULL: that pack gets the new bytes, the filter's other packs keep their old ones
    arg = dict(tap='fwd_tap_major', chan='fwd_chan_major', dgrad='dgrad_packed')
    for k in packs:
        mine = {j: t.clone() for j, t in old.items()}
        qp, qg, qm, qv = dev(p, g, m, v)
        extra = dict(ci0=ci0, n_dgrad=n) if k == 'dgrad' else {}
        ops.adam_step_conv(qp, qg, qm, qv, weight_decay=0.01, step=1000, dtype=dtype, **{arg[k]: mine[k]}, **extra, **HYPER)
        assert torch.equal(qp, tp), k
        for j in packs:
            assert torch.equal(mine[j], fresh[j] if j == k else old[j]), (k, j)
    # the flat form, held to the float64 bounds above, is the same arithmetic bit for bit
    fp, fg, fm, fv = dev(p, g, m, v)
    ops.adam_step(fp, fg, fm, fv, weight_decay=0.01, step=1000, **HYPER)
    assert torch.equal(fp, tp) and torch.equal(fm, tm) and torch.equal(fv, tv)


def test_conv_step_checks_arguments():
    p, g, m, v = dev(*make_inputs((32, 16, 3, 3), 5, 1))
    packs = make_packs(p, torch.float32, 8, 8)
    with pytest.raises(ValueError):
        ops.adam_step_conv(p, g, m, v, step=1, dgrad_packed=packs['dgrad'], ci0=9, n_dgrad=8)      # ci0 + n > c_in
    with pytest.raises(ValueError):
        ops.adam_step_conv(p, g, m, v, step=1, fwd_tap_major=packs['tap'][:-4])                    # not this filter's pack
    with pytest.raises(ValueError):
        ops.adam_step_conv(p, g, m, v, step=1, dtype=torch.float16)
    with pytest.raises(ValueError):
        ops.adam_step_conv(p.view(32, 16 * 9), g.view(32, 16 * 9), m.view(32, 16 * 9), v.view(32, 16 * 9), step=1)


# ----------------------------------------------------------------------------- the optimizer inside train_step
HC, T = 64, 5
CFG = types.SimpleNamespace(seq_len=T, flow_h=28, l_s=0.7, l_t=1.0, l_m=0.01, mm_th=0.15)
LR = 1e-4


def make_cell(precision):
    cell = ConvLSTMCell(HC, HC, precision=precision)
    cell.load_state_dict({k: torch.from_numpy(v) for k, v in synth.clstm_state(seed=11, input_size=HC, hidden_size=HC).items()})
    return cell.to(DEV)


def batch(it):
    seq = [torch.from_numpy(hashrng.uniform(9300 + 10 * it + t, (1, 6, HC, 7, 7), 0.0, 4.0)) for t in range(T)]
    flow = [torch.from_numpy(hashrng.normal(9400 + 10 * it + t, (1, 28, 56, 2), 0.0, 0.4)) for t in range(T)]
    return seq, flow


class PackCounter:
    """Counts the calls of the two pack entry points while it is installed on the loaded library."""

    def __init__(self, monkeypatch):
        self.calls = 0
        L = _lib.lib()
        for name in ('cp360_conv_pack_weights', 'cp360_train_dgrad_pack'):
            monkeypatch.setattr(L, name, self._wrap(getattr(L, name)))

    def _wrap(self, fn):
        def counted(*a):
            self.calls += 1
            return fn(*a)
        return counted


def plan_ptrs(plan):
    ptrs = {k: plan[k].packed.data_ptr() for k in ('d1', 'd2', 'dg')}
    for c in ('c1', 'c2', 'g'):
        ptrs.update({(c, lay): t.data_ptr() for lay, t in plan[c]._packed.items()})
    return ptrs


def assert_packs_current(cell, dtype, forward_packs=True):
    """Every pack of the training plan equals what the packers make of the parameters as they are now (forward_packs: a
    forward has run on this plan, so each convolution holds at least one forward layout)."""
    plan = trainer_of(cell).plans()
    hc = cell.hidden_size
    for conv, dg, w, ci0, n in ((plan['c1'], plan['d1'], cell.Conv1.weight, hc, hc), (plan['c2'], plan['d2'], cell.Conv2.weight, 0, 4 * hc),
                                (plan['g'], plan['dg'], cell.Gates.weight, 0, 4 * hc)):
        fresh = make_packs(w.detach(), dtype, ci0, n)
        assert conv._packed or not forward_packs, 'no forward pack'
        for lay, t in conv._packed.items():
            assert torch.equal(t, fresh['chan' if lay else 'tap']), (conv.tag, lay)
        assert torch.equal(dg.packed, fresh['dgrad']), conv.tag
    assert torch.equal(plan['c1'].bias, cell.Conv1.bias) and torch.equal(plan['c2'].bias, cell.Conv2.bias)
    assert torch.equal(plan['gbias'], cell.Gates.bias)


def test_fused_step_matches_torch_and_keeps_the_packs(monkeypatch):
    ct, cf = make_cell('fp32'), make_cell('fp32')
    ot, of = torch.optim.Adam(ct.parameters(), lr=LR), tt.FusedAdam(cf, lr=LR)
    p0 = {k: v.detach().cpu().numpy().copy() for k, v in cf.named_parameters()}
    seq, flow = batch(0)
    seen = {}
    real_step = of.step

    def spying_step(*a, **k):
        seen['plan'] = trainer_of(cf).plans()
        seen['ptrs'] = plan_ptrs(seen['plan'])
        return real_step(*a, **k)
    of.step = spying_step
    tt.train_step(ct, seq, flow, ot, CFG)
    tt.train_step(cf, seq, flow, of, CFG)
    of.step = real_step
    for (k, a), b in zip(ct.named_parameters(), cf.parameters()):
        assert torch.equal(a.grad, b.grad), k                                    # bit-reproducible gradients: both saw the same
        g = b.grad.cpu().numpy()
        z = np.zeros_like(g)
        want = adam64(p0[k], g, z, z, weight_decay=0.0, step=1, lr=LR, betas=(0.9, 0.999), eps=1e-8)
        assert_step((b.detach().cpu().numpy(), of.state[b]['exp_avg'].cpu().numpy(), of.state[b]['exp_avg_sq'].cpu().numpy()),
                    want, 'FusedAdam ' + k)
        assert_step((a.detach().cpu().numpy(), ot.state[a]['exp_avg'].cpu().numpy(), ot.state[a]['exp_avg_sq'].cpu().numpy()),
                    want, 'torch.optim.Adam ' + k)
        assert not np.array_equal(b.detach().cpu().numpy(), p0[k]), k
    tr = trainer_of(cf)
    assert tr.plans() is seen['plan'] and plan_ptrs(tr.plans()) == seen['ptrs']  # the same pack tensors, no repack
    assert_packs_current(cf, torch.float32)

    # the next iteration: no pack kernel after the fused step, six after torch's
    counter = PackCounter(monkeypatch)
    seq, flow = batch(1)
    tt.train_step(cf, seq, flow, of, CFG)
    assert counter.calls == 0
    assert plan_ptrs(tr.plans()) == seen['ptrs']
    tt.train_step(ct, seq, flow, ot, CFG)
    assert counter.calls >= 6
    monkeypatch.undo()

    # inference holds its own packs under the version rule: it repacks, and computes what a fresh cell of these weights does
    x = torch.from_numpy(hashrng.uniform(9500, (6, HC, 7, 7), 0.0, 1.0)).to(DEV)
    old_plan = cf.plans()
    h_before, _ = cf(x)
    counter = PackCounter(monkeypatch)
    tt.train_step(cf, seq, flow, of, CFG)
    assert counter.calls == 0
    assert cf.plans() is not old_plan
    h, c = cf(x)
    fresh = ConvLSTMCell(HC, HC, precision='fp32').to(DEV)
    fresh.load_state_dict(cf.state_dict())
    h2, c2 = fresh(x)
    assert torch.equal(h, h2) and torch.equal(c, c2) and not torch.equal(h, h_before)


def test_fused_bf16_packs_stay_equal_to_the_packers():
    cell = make_cell('bf16')
    opt = tt.FusedAdam(cell, lr=LR, weight_decay=0.01)
    for it in range(3):
        seq, flow = batch(it)
        tt.train_step(cell, seq, flow, opt, CFG)
        assert trainer_of(cell).current()
        assert_packs_current(cell, torch.bfloat16)
    assert int(opt.state[cell.Conv2.weight]['step'].item()) == 3


def test_fused_skips_parameters_without_gradient_and_stale_plans():
    cell = make_cell('fp32')
    opt = tt.FusedAdam(cell, lr=LR)
    seq, flow = batch(0)
    tt.train_step(cell, seq, flow, opt, CFG)
    # a parameter without .grad is skipped, as torch does
    w = cell.Conv2.weight.detach().clone()
    ver = cell.Conv2.weight._version
    cell.Conv2.weight.grad = None
    opt.step()
    assert torch.equal(cell.Conv2.weight, w) and cell.Conv2.weight._version == ver
    assert int(opt.state[cell.Conv2.weight]['step'].item()) == 1 and int(opt.state[cell.Conv1.weight]['step'].item()) == 2
    assert_packs_current(cell, torch.float32)
    # a plan that was stale before the step is not adopted: the lazy rule repacks it
    tr = trainer_of(cell)
    old = tr.plans()
    with torch.no_grad():
        cell.Conv1.weight.mul_(1.0)
    assert not tr.current()
    opt.step()
    assert not tr.current() and tr.plans() is not old
    assert_packs_current(cell, torch.float32, forward_packs=False)


# Step 3's loss terms of FusedAdam against torch.optim.Adam's, fp32.  Measured on one MI355X: relative
# differences 2.0e-7, 0 and 7.9e-8; the assertion is 4 x the largest, rounded up to a power of ten (never looser than 1e-4).
TRAJECTORY_RTOL = 1e-6


def test_fused_trajectory_follows_torch():
    ct, cf = make_cell('fp32'), make_cell('fp32')
    ot, of = torch.optim.Adam(ct.parameters(), lr=LR), tt.FusedAdam(cf, lr=LR)
    for it in range(3):
        seq, flow = batch(it)
        lt = [float(x) for x in tt.train_step(ct, seq, flow, ot, CFG)]
        lf = [float(x) for x in tt.train_step(cf, seq, flow, of, CFG)]
    rel = [abs(a - b) / abs(a) for a, b in zip(lt, lf)]
    print('step 3 loss terms: torch %r fused %r relative difference %r' % (lt, lf, rel))
    assert TRAJECTORY_RTOL <= 1e-4
    assert max(rel) <= TRAJECTORY_RTOL
