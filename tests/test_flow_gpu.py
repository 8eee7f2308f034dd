"""The flow resize and the fused flow loss on the GPU (csrc/flow_loss.hip, temporal_model/train_temporal.py resize_flow /
device_flow_losses): the resize against the numpy restatement of cv2 INTER_CUBIC (tests/flow_restate.py), the loss and its
gradient against the torch ``flow_losses`` on the CPU in float64, determinism, and train_step from flow at the reference's
resolution against a CPU pipeline (torch-CPU autograd cell, numpy resize, ``flow_losses``)."""
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

from cp_360_weakly_supervised_saliency_amd.model.clstm_train import window_maps
from cp_360_weakly_supervised_saliency_amd.temporal_model import train_temporal as tt
from cp_360_weakly_supervised_saliency_amd.utils import hashrng, synth
from tests import flow_restate as fr
from tests.test_train_cpu import golden, golden_batch
from tests.test_train_gpu import NAMES, make_cell, ref_cell, ref_window, rel

pytestmark = pytest.mark.gpu
DEV = 'cuda'
WEIGHTS = (0.7, 1.0, 0.01)            # l_s, l_t, l_m of the reference's config


def mixed_flow(seed, shape, small=0.12, large=8.0):
    """Flow whose magnitudes straddle mm_th = 0.15 (most pixels) with one pixel in ten moved by several pixels, so that
    warps near the border sample outside [-1, 1] (zero padding)."""
    n = hashrng.normal(seed, shape)
    u = hashrng.uniform(seed + 1, tuple(shape[:-1]) + (1,))
    return (n * np.where(u < 0.1, large, small)).astype(np.float32)


def loss_cfg(h, L):
    """The cfg that makes ``flow_losses`` read flows [B, L, h, 2h] as the pairs of the loss (seq_len = L + 1)."""
    return types.SimpleNamespace(flow_h=h, mm_th=0.15, seq_len=L + 1)


def cpu_losses(maps, flow_scaled, L, criterion=None):
    """flow_losses in float64 on the CPU for already-scaled flow [B, L, h, 2h, 2]: it multiplies by flow_h / W = 0.5 itself."""
    h = flow_scaled.shape[2]
    return tt.flow_losses(maps, 2.0 * flow_scaled, loss_cfg(h, L), L, criterion)


# ----------------------------------------------------------------------------- resize
RESIZE_CASES = [((480, 960), 240), ((480, 960), 28), ((480, 960), 480), ((240, 480), 480), ((480, 640), 240)]


@pytest.mark.parametrize('hw,flow_h', RESIZE_CASES)
def test_resize_matches_restatement(hw, flow_h):
    """cv2.resize(INTER_CUBIC) * flow_h / W against the float64 restatement; identity sizes: the scale alone, bit for bit.
    Bound: 3e-7 * max|flow| (twice the worst measured on the MI355X: 1.4e-7, the 2x upscale)."""
    flow = hashrng.normal(9300 + flow_h, (3,) + hw + (2,), 0, 2.0)
    got = tt.resize_flow(torch.from_numpy(flow).to(DEV), flow_h).cpu().numpy()
    want = fr.resize_flow(flow, flow_h)
    assert got.shape == (3, flow_h, 2 * flow_h, 2)
    err = float(np.max(np.abs(got - want)) / np.max(np.abs(flow)))
    print('resize %s -> %dx%d: max|d| / max|flow| = %.2e' % (hw, flow_h, 2 * flow_h, err))
    assert err <= 3e-7
    if hw == (flow_h, 2 * flow_h):
        np.testing.assert_array_equal(got, np.float32(flow_h / float(hw[1])) * flow)


# ----------------------------------------------------------------------------- loss forward / backward vs flow_losses
def loss_case(B, h, seed, L=3, w=7):
    maps = hashrng.uniform(seed, (B, L + 1, 2 * w, 4 * w), 0.0, 1.0)
    flow = mixed_flow(seed + 2, (B, L, h, 2 * h, 2))
    return maps, flow


@pytest.mark.parametrize('h', [28, 240, 480])
@pytest.mark.parametrize('B', [1, 4])
def test_loss_forward_backward_matches_flow_losses(B, h):
    """The three terms (rtol 1e-5) and d(0.7 sm + t + 0.01 m) / d maps (max|d| <= 1e-5 max|dmaps|) against torch autograd of
    flow_losses in float64; map 0 of each clip gets exactly zero."""
    L = 3
    maps, flow = loss_case(B, h, 9400 + h + B)
    st = np.sqrt(np.sum((flow.astype(np.float64)) ** 2, -1)) < 0.15
    assert 0.2 < st.mean() < 0.9                                 # both mask branches
    m64 = torch.from_numpy(maps).double().requires_grad_(True)
    want = cpu_losses(m64, torch.from_numpy(flow).double(), L)
    sum(wt * t for wt, t in zip(WEIGHTS, want)).backward()
    md = torch.from_numpy(maps).to(DEV).requires_grad_(True)
    got = tt.device_flow_losses(md, torch.from_numpy(flow).to(DEV), loss_cfg(h, L), L)
    sum(wt * t for wt, t in zip(WEIGHTS, got)).backward()
    g = np.array([t.item() for t in got])
    wv = np.array([t.item() for t in want])
    dm, wd = md.grad.cpu().numpy(), m64.grad.numpy()
    gerr = float(np.max(np.abs(dm - wd)) / np.max(np.abs(wd)))
    print('loss B=%d h=%d: terms rel %s, dmaps max|d| / max|g| %.2e' % (B, h, np.abs(g / wv - 1), gerr))
    np.testing.assert_allclose(g, wv, rtol=1e-5, atol=0)
    assert gerr <= 1e-5
    assert np.all(dm[:, 0] == 0)
    assert np.max(np.abs(wd[:, 1:])) > 0


def test_loss_uses_zero_padding():
    """A flow that moves every pixel far out of the image: the warp is all zeros, so loss_sm = sum next^2 per pair."""
    L, h = 3, 28
    maps = hashrng.uniform(9450, (1, L + 1, 14, 28), 0.0, 1.0)
    flow = np.full((1, L, h, 2 * h, 2), 500.0, np.float32)
    got = tt.device_flow_losses(torch.from_numpy(maps).to(DEV), torch.from_numpy(flow).to(DEV), loss_cfg(h, L), L)
    want = cpu_losses(torch.from_numpy(maps).double(), torch.from_numpy(flow).double(), L)
    np.testing.assert_allclose([t.item() for t in got], [t.item() for t in want], rtol=1e-5)
    assert got[2].item() == 0.0                                  # nothing is static


def test_loss_is_deterministic():
    L, h = 3, 240
    maps, flow = loss_case(4, h, 9460)
    fd = torch.from_numpy(flow).to(DEV)
    out = []
    for _ in range(2):
        md = torch.from_numpy(maps).to(DEV).requires_grad_(True)
        t = tt.device_flow_losses(md, fd, loss_cfg(h, L), L)
        sum(wt * x for wt, x in zip(WEIGHTS, t)).backward()
        out.append((torch.stack(t).detach().cpu().numpy(), md.grad.cpu().numpy()))
    assert np.array_equal(out[0][0].view(np.uint32), out[1][0].view(np.uint32))
    assert np.array_equal(out[0][1].view(np.uint32), out[1][1].view(np.uint32))


# ----------------------------------------------------------------------------- train_step from flow at the reference's size
def cpu_train(sd_np, batches, cfg, L=3):
    """The reference's train() on the CPU: torch autograd cell, the numpy cv2 resize, flow_losses, Adam.  flow_losses rescales by
    flow_h / W_loss = 0.5 while the reference scales by flow_h / W_orig: it gets resized * (2 flow_h / W_orig)."""
    sd = {k: torch.from_numpy(sd_np[k]).clone().requires_grad_(True) for k in NAMES}
    opt = torch.optim.Adam([sd[k] for k in NAMES], lr=cfg.lr)
    res = []
    for seq, flow in batches:
        seq_t = torch.from_numpy(np.stack(seq, 1))
        T = seq_t.shape[1]
        first = T - L - 1
        ref_cell.acts = []
        maps = ref_window(sd, tt.normalize_batch(seq_t), tuple(range(first, T)))
        ref_cell.acts = []
        fl = np.stack(flow, 1)[:, first:first + L]
        r = fr.resize(fl, cfg.flow_h, 2 * cfg.flow_h) * (2 * cfg.flow_h / float(fl.shape[3]))
        terms = tt.flow_losses(maps, torch.from_numpy(r.astype(np.float32)), loss_cfg(cfg.flow_h, L), L)
        loss = cfg.l_s * terms[0] + cfg.l_t * terms[1] + cfg.l_m * terms[2]
        opt.zero_grad()
        loss.backward()
        res.append((np.array([t.item() for t in terms]), {k: sd[k].grad.numpy().copy() for k in NAMES}))
        opt.step()
    return res, {k: sd[k].detach().numpy() for k in NAMES}


def test_train_step_from_full_resolution_flow():
    """ConvLSTMCell(8, 8), B = 2, two Adam iterations of train_step on 480 x 960 flow with flow_h = 240 (the HIP resize and
    loss) against the CPU pipeline: loss terms, iteration-1 gradients, parameters after iteration 2 (the tolerances of
    test_small_training_matches_reference_train)."""
    g, cfg = golden()
    cfg = types.SimpleNamespace(**vars(cfg))
    cfg.flow_h = 240
    seed = int(g['seeds'][2])
    B, T = int(g['seeds'][3]), int(g['seeds'][4])
    batches = []
    for it in range(2):
        seq, _ = golden_batch(g, it)
        flow = [mixed_flow(9700 + 10 * it + t, (B, 480, 960, 2), small=0.5, large=12.0) for t in range(T)]
        batches.append((seq, flow))
    want, after = cpu_train(synth.clstm_state(seed=seed, input_size=8, hidden_size=8), batches, cfg)
    cell, _ = make_cell(8, seed, 'fp32')
    opt = torch.optim.Adam(cell.parameters(), lr=cfg.lr)
    errs = {}
    for it, (seq, flow) in enumerate(batches):
        terms = tt.train_step(cell, [torch.from_numpy(s) for s in seq], [torch.from_numpy(f) for f in flow], opt, cfg)
        errs['loss%d' % it] = rel(np.array([t.item() for t in terms]), want[it][0])
        if it == 0:
            errs['grad'] = max(rel(p.grad.cpu().numpy(), want[0][1][n]) for n, p in cell.named_parameters())
    errs['after'] = max(float(np.max(np.abs(p.detach().cpu().numpy() - after[n]))) for n, p in cell.named_parameters())
    print('train (8, 8), flow 480x960 at flow_h 240 vs CPU pipeline:', {k: '%.2e' % v for k, v in errs.items()})
    assert errs['loss0'] <= 1e-4 and errs['loss1'] <= 1e-4
    assert errs['grad'] <= 1e-3
    assert errs['after'] <= 1e-5


def gpu_frames(seq):
    s = torch.from_numpy(seq).to(DEV)
    B, T, _, C, w, _ = s.shape
    return tt.normalize_batch(s).permute(0, 1, 2, 4, 5, 3).reshape(B, T, 6 * w * w, C).contiguous()


def test_full_size_step_at_reference_flow():
    """Hc = 1000, bf16, B = 1, flow 480 x 960 at flow_h 480 (the reference's default): one train_step; its loss terms against
    flow_losses (float64, CPU) on the same maps (read back through window_maps first), finite gradients."""
    cell, _ = make_cell(1000, 2, 'bf16')
    cfg = types.SimpleNamespace(seq_len=5, flow_h=480, l_s=0.7, l_t=1.0, l_m=0.01, mm_th=0.15)
    seq = synth.cam_clip(9800, 5)[None]
    flow = mixed_flow(9810, (1, 5, 480, 960, 2), small=0.3, large=10.0)
    with torch.no_grad():
        maps = window_maps(cell, gpu_frames(seq), range(1, 5)).cpu().double()
    want = tt.flow_losses(maps, torch.from_numpy(flow).double(), cfg)
    opt = torch.optim.Adam(cell.parameters(), lr=1e-5)
    got = tt.train_step(cell, torch.from_numpy(seq), torch.from_numpy(flow), opt, cfg)
    g, wv = np.array([t.item() for t in got]), np.array([t.item() for t in want])
    print('full size bf16 at flow 480x960: terms rel %s' % np.abs(g / wv - 1))
    np.testing.assert_allclose(g, wv, rtol=1e-5, atol=0)
    for n, p in cell.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n


def test_custom_criterion_goes_through_torch():
    """A criterion other than the reference's sum-MSE runs flow_losses on the device-resized flow."""
    g, cfg = golden()
    cfg = types.SimpleNamespace(**vars(cfg))
    cfg.flow_h = 240
    seq, _ = golden_batch(g, 0)
    B, T = len(seq[0]), len(seq)
    flow = [mixed_flow(9900 + t, (B, 480, 960, 2), small=0.5, large=12.0) for t in range(T)]
    cell, _ = make_cell(8, int(g['seeds'][2]), 'fp32')
    crit = nn.L1Loss(reduction='sum')
    with torch.no_grad():
        maps = window_maps(cell, gpu_frames(np.stack(seq, 1)), range(1, T)).cpu().double()
    r = fr.resize(np.stack(flow, 1)[:, 1:4], 240, 480) * (2 * 240 / 960.0)
    want = tt.flow_losses(maps, torch.from_numpy(r), loss_cfg(240, 3), 3, crit)
    opt = torch.optim.SGD(cell.parameters(), lr=0.0)
    got = tt.train_step(cell, [torch.from_numpy(s) for s in seq], [torch.from_numpy(f) for f in flow], opt, cfg, criterion=crit)
    np.testing.assert_allclose([t.item() for t in got], [t.item() for t in want], rtol=1e-4, atol=0)
    for p in cell.parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all())
