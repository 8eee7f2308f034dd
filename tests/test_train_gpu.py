"""ConvLSTM training on the GPU (csrc/clstm_train.hip, model/clstm_train.py, temporal_model/train_temporal.py): every
backward kernel against torch-CPU f32 autograd (F.conv2d + the differentiable index-gather CubePad of the oracle), the
(8, 8) run against the reference's own train() (tests/golden/clstm_train.npz), the full-size gradient, determinism and a
trained checkpoint loaded into the inference engine."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import o_c2e, o_clstm, o_metrics
from oracle.o_resnet import cubepad_t
from cp_360_weakly_supervised_saliency_amd import ops
from cp_360_weakly_supervised_saliency_amd.model.clstm import ConvLSTMCell
from cp_360_weakly_supervised_saliency_amd.model.clstm_train import trainer_of, window_maps
from cp_360_weakly_supervised_saliency_amd.temporal_model import train_temporal as tt
from cp_360_weakly_supervised_saliency_amd.utils import hashrng, synth

from tests.test_train_cpu import golden, golden_batch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAMES = ('Conv1.weight', 'Conv1.bias', 'Conv2.weight', 'Conv2.bias', 'Gates.weight', 'Gates.bias')


# ----------------------------------------------------------------------------- torch-CPU f32 autograd references
def conv_pad(x, w, b=None):
    return F.conv2d(cubepad_t(x, 1), w, b)


def ref_cell(sd, x, h, c):
    a1 = F.relu(conv_pad(torch.cat((x, h), 1), sd['Conv1.weight'], sd['Conv1.bias']))
    a2 = F.relu(conv_pad(a1, sd['Conv2.weight'], sd['Conv2.bias']))
    i, f, o, g = conv_pad(a2, sd['Gates.weight'], sd['Gates.bias']).chunk(4, 1)
    c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
    ref_cell.acts.append((a1.detach(), a2.detach()))
    return torch.sigmoid(o) * torch.tanh(c), c


ref_cell.acts = []


_C2E = {}


def ref_map(h6, w):
    """to_equi_nn + channel max of one clip's hidden [6, C, w, w] (differentiable, zero padding, align_corners False)."""
    if w not in _C2E:
        fm, coord = o_c2e.c2e_tables(w)
        pc = o_c2e.sample_pixel_coords(coord, w).reshape(-1, 2)
        x0, y0 = np.floor(pc[:, 0]), np.floor(pc[:, 1])
        fx, fy = (pc[:, 0] - x0).astype(np.float32), (pc[:, 1] - y0).astype(np.float32)
        idx, wts = [], []
        for k, wt in enumerate(((1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy)):
            xx, yy = x0.astype(np.int64) + (k & 1), y0.astype(np.int64) + (k >> 1)
            ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < w)
            idx.append(torch.from_numpy((fm.reshape(-1) * w + np.clip(yy, 0, w - 1)) * w + np.clip(xx, 0, w - 1)))
            wts.append(torch.from_numpy(np.where(ok, wt, 0).astype(np.float32)))
        _C2E[w] = (idx, wts)
    idx, wts = _C2E[w]
    flat = h6.permute(0, 2, 3, 1).reshape(6 * w * w, -1)
    out = sum(flat[idx[k]] * wts[k][:, None] for k in range(4))
    return out.max(dim=1).values.view(2 * w, 4 * w)


def ref_window(sd, frames, map_steps):
    """frames [B, T, 6, C, w, w] (normalised) -> maps [B, n, 2w, 4w] (train_temporal.py:87-107)."""
    B, T, _, C, w, _ = frames.shape
    x = [frames[:, t].reshape(6 * B, C, w, w) for t in range(T)]
    h = c = x[0]
    maps = {}
    for t in range(T):
        h, c = ref_cell(sd, x[t], h, c)
        if t in map_steps:
            maps[t] = torch.stack([ref_map(h[6 * b:6 * b + 6], w) for b in range(B)])
    return torch.stack([maps[t] for t in map_steps], 1)


def ref_grads(sd_np, frames_np, map_steps, dmaps_np):
    sd = {k: torch.from_numpy(v).clone().requires_grad_(True) for k, v in sd_np.items()}
    ref_cell.acts = []
    maps = ref_window(sd, torch.from_numpy(frames_np), map_steps)
    (maps * torch.from_numpy(dmaps_np)).sum().backward()
    acts = [(a1.permute(0, 2, 3, 1).numpy() > 0, a2.permute(0, 2, 3, 1).numpy() > 0) for a1, a2 in ref_cell.acts]
    ref_cell.acts = []
    return maps.detach().numpy(), {k: sd[k].grad.numpy() for k in NAMES}, acts


def gpu_grads(cell, frames_np, map_steps, dmaps_np):
    B, T, _, C, w, _ = frames_np.shape
    fr = torch.from_numpy(np.ascontiguousarray(frames_np.transpose(0, 1, 2, 4, 5, 3)).reshape(B, T, 6 * w * w, C)).to(DEV)
    for p in cell.parameters():
        p.grad = None
    maps = window_maps(cell, fr, map_steps)
    maps.backward(torch.from_numpy(dmaps_np).to(DEV))
    return maps.detach().cpu().numpy(), {k: p.grad.cpu().numpy() for k, p in cell.named_parameters()}


def rel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30))


def cos(a, b):
    a, b = a.reshape(-1).astype(np.float64), b.reshape(-1).astype(np.float64)
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)))


def make_cell(hc, seed, precision):
    cell = ConvLSTMCell(hc, hc, precision=precision)
    sd = synth.clstm_state(seed=seed, input_size=hc, hidden_size=hc)
    cell.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return cell.to(DEV), sd


# ----------------------------------------------------------------------------- single kernels
def test_gates_forward_and_backward():
    M, hc = 12 * 49, 24
    pre = torch.from_numpy(hashrng.normal(8100, (M, 4 * hc), 0, 1.5))
    bias = torch.from_numpy(hashrng.normal(8101, (4 * hc,), 0, 0.3))
    c_prev = torch.from_numpy(hashrng.normal(8102, (M, hc)))
    dh_np, dc_np = hashrng.normal(8103, (M, hc)), hashrng.normal(8104, (M, hc))
    g = (pre + bias).requires_grad_(True)
    cp = c_prev.clone().requires_grad_(True)
    i, f, o, gg = g.chunk(4, 1)
    c = torch.sigmoid(f) * cp + torch.sigmoid(i) * torch.tanh(gg)
    h = torch.sigmoid(o) * torch.tanh(c)
    (h * torch.from_numpy(dh_np) + c * torch.from_numpy(dc_np)).sum().backward()
    d = lambda a: a.to(DEV).contiguous()
    c_next = torch.empty(M, hc, device=DEV)
    h_f32 = torch.empty(M, hc, device=DEV)
    h_out = torch.empty(M, 2 * hc, device=DEV)
    acts = torch.empty(M, 4 * hc, device=DEV)
    ops.train_gates(d(pre), 1, d(bias), d(c_prev), c_next, h_out, hc, h_f32, acts, M, hc)
    assert rel(h_f32.cpu().numpy(), h.detach().numpy()) <= 1e-6 and rel(c_next.cpu().numpy(), c.detach().numpy()) <= 1e-6
    assert torch.equal(h_out[:, hc:], h_f32)
    dc = d(torch.from_numpy(dc_np))
    dg = torch.empty(M, 4 * hc, device=DEV)
    ops.train_gates_backward(d(torch.from_numpy(dh_np)), dc, acts, d(c_prev), c_next, dg, M, hc)
    assert rel(dg.cpu().numpy(), g.grad.numpy()) <= 1e-5
    assert rel(dc.cpu().numpy(), cp.grad.numpy()) <= 1e-5


def dgrad_case(n6, face, c_in, c_out, ci0, n, dtype, seed, mask=True):
    """dX of CubePad(1) + 3x3 conv (channels [ci0, ci0 + n)) times the ReLU mask of a random activation, vs autograd."""
    x = torch.from_numpy(hashrng.normal(seed, (n6, c_in, face, face))).requires_grad_(True)
    w = torch.from_numpy(hashrng.normal(seed + 1, (c_out, c_in, 3, 3), 0, (2.0 / (9 * c_in)) ** 0.5))
    dy = hashrng.normal(seed + 2, (n6, c_out, face, face))
    act = hashrng.normal(seed + 3, (n6, face, face, n))
    rb = (lambda a: a.to(torch.bfloat16).float()) if dtype == torch.bfloat16 else (lambda a: a)
    conv_pad(x, rb(w)).mul(rb(torch.from_numpy(dy))).sum().backward()
    want = x.grad[:, ci0:ci0 + n].permute(0, 2, 3, 1).numpy()
    if mask:
        want = np.where(rb(torch.from_numpy(act)).numpy() > 0, want, 0)
    pack = ops.DgradPack(w.to(DEV), ci0, n, dtype)
    dy_d = ops.nchw_to_nhwc(torch.from_numpy(dy).to(DEV), out_dtype=dtype)
    off, ent = ops.cubepad_inverse(face)
    out = torch.empty((n6, face, face, n), dtype=dtype, device=DEV)
    ops.cubepad_adjoint(pack.dgrad(dy_d), torch.from_numpy(off).to(DEV), torch.from_numpy(ent).to(DEV), out,
                        act=torch.from_numpy(act).to(DEV, dtype) if mask else None)
    return out.float().cpu().numpy(), want


@pytest.mark.parametrize('face', [1, 2, 7])
def test_dgrad_small_corner_heavy(face):
    """Faces of 1 and 2 pixels: every pixel is a corner with several CubePad copies."""
    got, want = dgrad_case(12, face, 16, 32, 0, 16, torch.float32, 8200 + face)
    assert rel(got, want) <= 1e-5, rel(got, want)
    got, want = dgrad_case(12, face, 16, 32, 0, 16, torch.bfloat16, 8210 + face)
    assert rel(got, want) <= 2e-2 and cos(got, want) >= 0.9999


def test_dgrad_full_conv2_and_conv1_hidden_half():
    got, want = dgrad_case(6, 7, 4000, 4000, 0, 4000, torch.float32, 8300)
    print('dgrad Conv2 4000->4000 fp32: rel %.2e' % rel(got, want))
    assert rel(got, want) <= 1e-4
    got, want = dgrad_case(6, 7, 2000, 4000, 1000, 1000, torch.float32, 8310, mask=False)
    print('dgrad Conv1 hidden half fp32: rel %.2e' % rel(got, want))
    assert rel(got, want) <= 1e-4


def wgrad_case(n6, face, c_in, ld, c_out, dtype, seed):
    x_np = hashrng.normal(seed, (n6, ld, face, face))
    dy_np = hashrng.normal(seed + 1, (n6, c_out, face, face))
    rb = (lambda a: a.to(torch.bfloat16).float()) if dtype == torch.bfloat16 else (lambda a: a)
    w = torch.zeros(c_out, c_in, 3, 3, requires_grad=True)
    b = torch.zeros(c_out, requires_grad=True)
    conv_pad(rb(torch.from_numpy(x_np))[:, :c_in], w, b).mul(rb(torch.from_numpy(dy_np))).sum().backward()
    dw = torch.empty(c_out, c_in, 3, 3, device=DEV)
    db = torch.empty(c_out, device=DEV)
    tab = torch.from_numpy(ops.cubepad_table(face, 1)).to(DEV)
    ops.conv_wgrad(ops.nchw_to_nhwc(torch.from_numpy(dy_np).to(DEV), out_dtype=dtype),
                   ops.nchw_to_nhwc(torch.from_numpy(x_np).to(DEV), out_dtype=dtype), c_in, tab, dw, db)
    return dw.cpu().numpy(), db.cpu().numpy(), w.grad.numpy(), b.grad.numpy()


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_wgrad_small(dtype):
    gw, gb, ww, wb = wgrad_case(24, 7, 16, 20, 32, dtype, 8400)               # 4 "steps" of one clip; x wider than c_in
    print('wgrad small %s: rel %.2e / %.2e, max|g| %.3e' % (dtype, rel(gw, ww), rel(gb, wb), np.max(np.abs(ww))))
    assert np.max(np.abs(ww)) > 1 and np.max(np.abs(wb)) > 1
    assert rel(gw, ww) <= 1e-5 and rel(gb, wb) <= 1e-5, (rel(gw, ww), rel(gb, wb))


def test_wgrad_full_conv2():
    gw, gb, ww, wb = wgrad_case(6, 7, 4000, 4000, 4000, torch.float32, 8500)
    print('wgrad Conv2 4000->4000 fp32: rel %.2e / %.2e, max|g| %.3e / %.3e, bit-equal %.4f' % (
        rel(gw, ww), rel(gb, wb), np.max(np.abs(ww)), np.max(np.abs(wb)), np.mean(gw == ww)))
    assert np.max(np.abs(ww)) > 1 and np.max(np.abs(wb)) > 1
    assert rel(gw, ww) <= 1e-4 and rel(gb, wb) <= 1e-5


def test_saliency_forward_and_backward():
    B, C, w = 2, 40, 7
    h = torch.from_numpy(hashrng.normal(8600, (6 * B, C, w, w))).requires_grad_(True)
    dmap = torch.from_numpy(hashrng.normal(8601, (B, 2 * w, 4 * w)))
    maps = torch.stack([ref_map(h[6 * b:6 * b + 6], w) for b in range(B)])
    (maps * dmap).sum().backward()
    c2e = trainer_of(make_cell(8, 1, 'fp32')[0]).tables(w, torch.device(DEV))
    hd = ops.nchw_to_nhwc(h.detach().to(DEV))
    mx = torch.empty(B, 2 * w, 4 * w, device=DEV)
    am = torch.empty(B, 2 * w, 4 * w, dtype=torch.int32, device=DEV)
    ops.saliency_forward(hd, c2e['fm'], c2e['pc'], mx, am)
    assert np.max(np.abs(mx.cpu().numpy() - maps.detach().numpy())) <= 1e-5
    dh = torch.zeros(6 * B, w, w, C, device=DEV)
    ops.saliency_backward(dmap.to(DEV), am, c2e['pc'], c2e['c2e_off'], c2e['c2e_ent'], dh)
    assert rel(dh.cpu().numpy(), h.grad.permute(0, 2, 3, 1).numpy()) <= 1e-5


# ----------------------------------------------------------------------------- the reference's train(), end to end
def test_small_training_matches_reference_train():
    """ConvLSTMCell(8, 8), B = 2, two iterations of train_step with Adam: loss terms, iteration-1 gradients and the
    parameters after iteration 2 against the reference's train() on the CPU."""
    g, cfg = golden()
    cell, _ = make_cell(8, int(g['seeds'][2]), 'fp32')
    opt = torch.optim.Adam(cell.parameters(), lr=cfg.lr)
    errs = {}
    for it in range(2):
        seq, flow = golden_batch(g, it)
        terms = tt.train_step(cell, [torch.from_numpy(s) for s in seq], [torch.from_numpy(f) for f in flow], opt, cfg)
        errs['loss%d' % it] = rel(np.array([t.item() for t in terms]), g['losses'][it])
        if it == 0:
            errs['grad'] = max(rel(p.grad.cpu().numpy(), g['grad_' + n]) for n, p in cell.named_parameters())
    errs['after'] = max(float(np.max(np.abs(p.detach().cpu().numpy() - g['after_' + n]))) for n, p in cell.named_parameters())
    print('train (8, 8) vs reference:', {k: '%.2e' % v for k, v in errs.items()})
    assert errs['loss0'] <= 1e-4 and errs['loss1'] <= 1e-4
    assert errs['grad'] <= 1e-3
    assert errs['after'] <= 1e-5


# ----------------------------------------------------------------------------- full size
FULL_STEPS = (1, 2, 3, 4)


@pytest.fixture(scope='module')
def full_case():
    hc, T = 1000, 5
    sd = synth.clstm_state(seed=2, input_size=hc, hidden_size=hc)
    frames = synth.cam_clip(8700, T)[None]                                   # [1, T, 6, C, 7, 7]
    frames = ((frames - frames.min()) / (frames - frames.min()).max()).astype(np.float32)
    dmaps = hashrng.normal(8701, (1, len(FULL_STEPS), 14, 28), 0, 1.0)
    maps, grads, acts = ref_grads(sd, frames, FULL_STEPS, dmaps)
    return sd, frames, dmaps, maps, grads, acts


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_full_size_gradients(full_case, precision):
    """Hc = 1000, B = 1, T = 5: every parameter's gradient against torch-CPU f32 autograd.  max|d| / max|g| is dominated by
    ReLU decisions that the two f32 forwards take on opposite sides of zero (their number is logged): one flipped element of
    a1 / a2 moves whole rows of dW1 / dW2 by one product, while the Gates gradient, upstream of every ReLU, agrees to 2e-5.
    Bounds: about twice the worst measured on the MI355X (fp32: 5.1e-3, cosine 1 - 8e-8; bf16: 9.5e-2, cosine 1 - 1.5e-3)."""
    sd, frames, dmaps, want_maps, want, ref_acts = full_case
    cell = ConvLSTMCell(1000, 1000, precision=precision)
    cell.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    cell.to(DEV)
    maps, got = gpu_grads(cell, frames, FULL_STEPS, dmaps)
    res = {n: (rel(got[n], want[n]), cos(got[n], want[n])) for n in NAMES}
    fr = torch.from_numpy(np.ascontiguousarray(frames.transpose(0, 1, 2, 4, 5, 3)).reshape(1, 5, 294, 1000)).to(DEV)
    _, saved = trainer_of(cell).forward(fr, FULL_STEPS)
    flips = sum(int(np.sum((saved[k][t].float().cpu().numpy() > 0) != ref_acts[t][j]))
                for t in range(5) for j, k in enumerate(('a1', 'a2')))
    print('full size %s: maps max|d| %.2e; ReLU decisions flipped vs CPU: %d of %d;' % (
        precision, np.max(np.abs(maps - want_maps)), flips, 2 * 5 * 294 * 4000),
        ' '.join('%s %.2e/%.8f' % (n, a, c) for n, (a, c) in res.items()))
    if precision == 'fp32':
        assert np.max(np.abs(maps - want_maps)) <= 1e-3
        assert res['Gates.weight'][0] <= 1e-3 and res['Gates.bias'][0] <= 1e-3
        assert all(a <= 1e-2 and c >= 0.9999 for a, c in res.values()), res
    else:
        assert all(a <= 0.2 and c >= 0.997 for a, c in res.values()), res

    # determinism: the same iteration again gives the same bits
    _, again = gpu_grads(cell, frames, FULL_STEPS, dmaps)
    assert all(np.array_equal(got[n], again[n]) for n in NAMES)


def test_trained_checkpoint_loads_into_engine():
    """Three bf16 iterations at full size, state_dict(), a strict SaliencyEngine load: its map equals the oracle's window
    saliency with the updated weights (fp32 engine: 1e-3; AUC-Judd / CC within 1e-3)."""
    from cp_360_weakly_supervised_saliency_amd.pipeline import SaliencyEngine
    cell, sd0 = make_cell(1000, 2, 'bf16')
    opt = torch.optim.Adam(cell.parameters(), lr=1e-5)
    cfg = types.SimpleNamespace(seq_len=5, flow_h=28, l_s=0.7, l_t=1.0, l_m=0.01, mm_th=0.15)
    for it in range(3):
        seq = torch.from_numpy(synth.cam_clip(8800 + it, 5))[None]               # [1, T, 6, C, 7, 7]
        flow = torch.from_numpy(hashrng.normal(8810 + it, (1, 5, 28, 56, 2), 0, 0.5))
        tt.train_step(cell, seq.unbind(1), flow.unbind(1), opt, cfg)
    sd = {k: v.detach().cpu() for k, v in cell.state_dict().items()}
    assert set(sd) == set(sd0) and any(not np.array_equal(sd[k].numpy(), sd0[k]) for k in sd)
    T = 5
    eng = SaliencyEngine(synth.resnet50_state(seed=1), sd, (448, 896), 224, clips=1, frames=T, precision='fp32')
    frames = synth.cam_clip(8900, T)
    cam = torch.from_numpy(np.ascontiguousarray(frames.transpose(0, 1, 3, 4, 2)).reshape(1, T, 294, 1000)).to(DEV)
    sal = eng.temporal_stage(cam).cpu().numpy()[0]
    ref = o_clstm.window_saliency(frames, sd)
    fix = synth.fixations_from_map(ref, 151, 14 * 16, 28 * 16)
    auc = o_metrics.auc_judd(sal, fix, rng=np.random.RandomState(0)) - o_metrics.auc_judd(ref, fix, rng=np.random.RandomState(0))
    cc = o_metrics.corr_coeff(sal, fix) - o_metrics.corr_coeff(ref, fix)
    print('trained checkpoint in the engine: max|d| %.2e dAUC %.2e dCC %.2e' % (np.max(np.abs(sal - ref)), auc, cc))
    assert np.max(np.abs(sal - ref)) <= 1e-3
    assert abs(auc) <= 1e-3 and abs(cc) <= 1e-3
