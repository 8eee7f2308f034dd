"""CPU tests of the fused Adam step (include/cp360.h "K5o", ops.adam_step, train_temporal.FusedAdam): the optimizer's state
interchanges with torch.optim.Adam, what it does not implement is refused, nothing runs without a GPU, and the header, the
binding and the library agree on the two entry points."""
import ctypes as C
import os
import re

import pytest
import torch

from cp_360_weakly_supervised_saliency_amd import _lib, ops
from cp_360_weakly_supervised_saliency_amd.model.clstm import ConvLSTMCell
from cp_360_weakly_supervised_saliency_amd.model.clstm_train import trainer_of
from cp_360_weakly_supervised_saliency_amd.temporal_model import train_temporal as tt

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADAM_SYMBOLS = ['cp360_train_adam', 'cp360_train_adam_conv']


def same(a, b):
    """Nested equality of two optimizer state dicts, tensors by value."""
    if torch.is_tensor(a) or torch.is_tensor(b):
        return torch.is_tensor(a) and torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return a == b


def with_state(opt, seed):
    """An optimizer state as three steps would leave it (written directly: no step runs on the CPU)."""
    gen = torch.Generator().manual_seed(seed)
    for group in opt.param_groups:
        for p in group['params']:
            opt.state[p] = dict(step=torch.tensor(3.0), exp_avg=torch.randn(p.shape, generator=gen),
                                exp_avg_sq=torch.rand(p.shape, generator=gen))
    return opt


def test_state_dict_round_trips_with_torch_adam():
    cell = ConvLSTMCell(8, 8)
    kw = dict(lr=3e-4, betas=(0.8, 0.99), eps=1e-7, weight_decay=0.01)
    fused, plain = tt.FusedAdam(cell, **kw), torch.optim.Adam(cell.parameters(), **kw)
    assert isinstance(fused, torch.optim.Optimizer)
    assert same(fused.state_dict(), plain.state_dict())                       # the same keys and values before any step
    assert set(fused.state_dict()['param_groups'][0]) == set(plain.state_dict()['param_groups'][0])
    # torch -> fused
    sd = with_state(plain, 1).state_dict()
    assert set(sd['state'][0]) == {'step', 'exp_avg', 'exp_avg_sq'}
    fused.load_state_dict(sd)
    assert same(fused.state_dict(), sd)
    assert torch.equal(fused.state[cell.Conv2.weight]['exp_avg'], plain.state[cell.Conv2.weight]['exp_avg'])
    # fused -> torch
    other = ConvLSTMCell(8, 8)
    sd = with_state(tt.FusedAdam(other, **kw), 2).state_dict()
    fresh = torch.optim.Adam(other.parameters())
    fresh.load_state_dict(sd)
    assert same(fresh.state_dict(), sd)
    assert fresh.param_groups[0]['lr'] == 3e-4 and fresh.param_groups[0]['betas'] == (0.8, 0.99)
    # schedulers and zero_grad are the base class's
    sched = torch.optim.lr_scheduler.StepLR(fused, step_size=1, gamma=0.5)
    assert sched.get_last_lr() == [3e-4]
    cell.Conv1.bias.grad = torch.ones_like(cell.Conv1.bias)
    fused.zero_grad()
    assert cell.Conv1.bias.grad is None


def test_refusals():
    cell = ConvLSTMCell(8, 8)
    for key in ('amsgrad', 'maximize', 'capturable'):
        with pytest.raises(ValueError, match=key):
            tt.FusedAdam(cell, **{key: True})
    opt = tt.FusedAdam(cell)
    with pytest.raises(ValueError, match='closure'):
        opt.step(lambda: 0.0)
    # a checkpoint of an Adam variant loads (the groups are torch's) but does not step
    sd = torch.optim.Adam(cell.parameters(), amsgrad=True).state_dict()
    opt.load_state_dict(sd)
    with pytest.raises(ValueError, match='amsgrad'):
        opt.step()
    opt = tt.FusedAdam(cell)
    w = cell.Conv1.bias
    w.grad = torch.sparse_coo_tensor(torch.tensor([[0]]), torch.tensor([1.0]), w.shape)
    with pytest.raises(ValueError, match='sparse'):
        opt.step()


def test_step_on_a_cpu_cell_raises():
    cell = ConvLSTMCell(8, 8)
    opt = tt.FusedAdam(cell)
    for p in cell.parameters():
        p.grad = torch.ones_like(p)
    before = [p.detach().clone() for p in cell.parameters()]
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        opt.step()
    assert all(torch.equal(a, b) for a, b in zip(before, cell.parameters())) and len(opt.state) == 0
    t = torch.zeros(8)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.adam_step(t, t, t, t)
    w = torch.zeros(32, 16, 3, 3)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.adam_step_conv(w, w, w, w)


def test_trainer_without_a_plan_is_not_current():
    tr = trainer_of(ConvLSTMCell(8, 8))
    assert not tr.current()
    tr.adopt()                                            # nothing to adopt: still no plan, no launch
    assert not tr.current()


def test_adam_entry_points_declared_and_bound():
    hdr = open(os.path.join(REPO, 'include', 'cp360.h')).read()
    sect = hdr[hdr.index('K5o: fused Adam'):hdr.index('K5f: flow resize and flow loss')]
    assert sorted(set(re.findall(r'\b(cp360_train_[a-z0-9_]+)\s*\(', sect))) == sorted(ADAM_SYMBOLS)
    assert set(ADAM_SYMBOLS) <= set(_lib.PUBLIC_SYMBOLS)
    L = _lib.lib()
    for name in ADAM_SYMBOLS:
        assert hasattr(L, name) and getattr(L, name).argtypes
    assert L.cp360_version() == _lib.ABI_VERSION == 306


def test_adam_entry_points_validate_without_gpu():
    L = _lib.lib()
    one = C.c_void_p(16)
    hyper = (1e-3, 0.9, 0.999, 1e-8, 0.0, 0.1, 0.0316)
    assert L.cp360_train_adam(one, one, one, one, 0, *hyper, None) == -1                       # n <= 0
    assert L.cp360_train_adam(one, one, one, one, -4, *hyper, None) == -1
    assert L.cp360_train_adam(one, None, one, one, 8, *hyper, None) == -5
    assert L.cp360_train_adam(one, one, C.c_void_p(20), one, 8, *hyper, None) == -6            # 16-byte accesses
    conv = lambda c_out, c_in, dtype, tap, chan, dg, ci0, n: L.cp360_train_adam_conv(one, one, one, one, c_out, c_in, *hyper,
                                                                                      dtype, tap, chan, dg, ci0, n, None)
    assert conv(0, 16, _lib.F32, None, None, None, 0, 0) == -1
    assert conv(32, 16, _lib.F32, None, None, one, 8, 9) == -1                                 # ci0 + n_dgrad > c_in
    assert conv(32, 16, _lib.F16, None, None, None, 0, 0) == -8                                # f32 / bf16 only
    assert conv(32, 16, _lib.U8, one, None, None, 0, 0) == -8
    assert conv(32, 18, _lib.F32, None, None, None, 0, 0) == -6                                # c_in % 4
    assert conv(65536, 4096, _lib.F32, None, None, None, 0, 0) == -8                           # 9 c_out c_in >= 2^31
    assert L.cp360_train_adam_conv(None, one, one, one, 32, 16, *hyper, _lib.F32, None, None, None, 0, 0, None) == -5
