"""Launch paths of the training kernels (csrc/clstm_train.hip "K5t", csrc/flow_loss.hip "K5f") that the shapes of the
trainer never reach: remainders, thresholds, optional arguments and mixed types admitted by include/cp360.h.  Every test
calls a kernel through ``ops`` (or ``train_temporal``) and compares with a plain float64 reference computed on the CPU
(torch autograd or numpy), never with another path of the library.  Inputs come from ``utils.hashrng``.

Bounds.  f32 paths keep the bounds of tests/test_train_gpu.py and tests/test_flow_gpu.py for the same kernel (gates 1e-6 /
1e-5, dgrad / wgrad / adjoint 1e-5 of max|reference|, saliency map 1e-5 absolute, loss terms rtol 1e-5, dmaps 1e-5 of max,
resize 3e-7 of max|flow|).  bf16 paths: the reference is the same operation in float64 on bf16-rounded operands, so what
remains is the f32 accumulation order (the f32 bound) plus, where the output itself is bf16, one rounding of it (2^-8
relative, elementwise): ``close_bf16``.

Decisions that are discontinuous are kept off the knife edge by construction and ASSERTED on the CPU before the GPU is
called: no flow magnitude within 1e-5 of mm_th (``gap_flow`` draws magnitudes outside [0.14, 0.16]), top-two channel gap of
the saliency argmax at least 1e-4 unless the tie is exact, ReLU operands exactly +-0 or at least 1e-3 in magnitude."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import o_c2e
from oracle.o_resnet import cubepad_t
from cp_360_weakly_supervised_saliency_amd import ops
from cp_360_weakly_supervised_saliency_amd.temporal_model import train_temporal as tt
from cp_360_weakly_supervised_saliency_amd.utils import hashrng
from cp_360_weakly_supervised_saliency_amd.utils.cube_to_equi import Cube2Equi
from tests import flow_restate as fr
from tests.test_train_gpu import rel

pytestmark = pytest.mark.gpu
DEV = 'cuda'
MM_TH = 0.15
WEIGHTS = (0.7, 1.0, 0.01)            # l_s, l_t, l_m of the reference's config
BF16_EPS = 2.0 ** -8                  # one round-to-nearest of a bf16 output, relative


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    return t.to(DEV, dtype).contiguous()


def rb(t):
    """bf16 rounding of a torch tensor, back in its own dtype (the operand a bf16 kernel reads)."""
    return t.to(torch.bfloat16).to(t.dtype)


def close_bf16(got, want, f32_bound):
    """max over elements of |got - want| / (2^-8 |want| + f32_bound max|want|): <= 1 when a bf16 output is one rounding away
    from a value that is itself within the f32 bound of the float64 reference."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.max(np.abs(got - want) / (BF16_EPS * np.abs(want) + f32_bound * np.max(np.abs(want)))))


# ============================================================================= K5f: flow loss
def gap_flow(seed, shape):
    """Scaled flow [..., 2] whose magnitudes avoid mm_th = 0.15 by construction: 45 % static in [0.01, 0.14], 45 % moving in
    [0.16, 0.6], 10 % moved by 2 .. 12 pixels (warps near the border sample outside the image: zero padding)."""
    lead = tuple(shape[:-1])
    u = hashrng.uniform(seed, lead, dtype=np.float64)
    v = hashrng.uniform(seed + 1, lead, dtype=np.float64)
    ang = hashrng.uniform(seed + 2, lead, 0.0, 2 * np.pi, dtype=np.float64)
    mag = np.where(u < 0.45, 0.01 + 0.13 * v, np.where(u < 0.9, 0.16 + 0.44 * v, 2.0 + 10.0 * v))
    return np.stack([mag * np.cos(ang), mag * np.sin(ang)], -1).astype(np.float32)


def loss_inputs(seed, B, L, w, h, wl):
    """maps [B, L + 1, 2w, 4w] in [0, 1) and scaled flow [B, L, h, wl, 2]; asserts the mask condition on the f32 values."""
    maps = hashrng.uniform(seed, (B, L + 1, 2 * w, 4 * w), 0.0, 1.0)
    flow = gap_flow(seed + 1, (B, L, h, wl, 2))
    mag = np.sqrt(np.sum(flow.astype(np.float64) ** 2, -1))
    assert np.min(np.abs(mag - MM_TH)) >= 1e-5                    # the mask decision is not on the knife edge
    assert 0.2 < np.mean(mag < MM_TH) < 0.8 or mag.size < 64      # both mask branches
    return maps, flow


def loss_ref(maps, flow, weights):
    """float64 terms and d(sum weights * terms) / d maps of tests/flow_restate.py loss_terms (pinned on the CPU against
    ``flow_losses`` by tests/test_flow_cpu.py)."""
    m = torch.from_numpy(maps).double().requires_grad_(True)
    terms = fr.loss_terms(m, torch.from_numpy(flow).double(), MM_TH)
    sum(wt * t for wt, t in zip(weights, terms)).backward()
    return np.array([t.item() for t in terms]), m.grad.numpy()


def check_loss(tag, maps, flow, weights=WEIGHTS):
    """ops.flow_loss_forward / backward against loss_ref: terms rtol 1e-5, dmaps 1e-5 of max|dmaps|, map 0 exactly zero."""
    wv, wd = loss_ref(maps, flow, weights)
    md, fd = dev(maps), dev(flow)
    g = ops.flow_loss_forward(md, fd, MM_TH).cpu().numpy().astype(np.float64)
    dm = ops.flow_loss_backward(md, fd, dev(np.float32(weights)), MM_TH).cpu().numpy()
    assert np.max(np.abs(wd[:, 1:])) > 0 and np.all(wv[:2] > 0)
    gerr = float(np.max(np.abs(dm - wd)) / np.max(np.abs(wd)))
    terr = np.abs(g - wv) / np.where(wv != 0, np.abs(wv), 1.0)
    print('loss %s: terms rel %s, dmaps max|d| / max|g| %.2e' % (tag, terr, gerr))
    np.testing.assert_allclose(g, wv, rtol=1e-5, atol=0)
    assert gerr <= 1e-5, gerr
    assert np.all(dm[:, 0] == 0)


@pytest.mark.parametrize('wl', [1024, 1025, 1200, 2048])
def test_loss_row_chunks(wl):
    """flow_loss_rows_kernel, second and later kRowChunk (1024) chunks of a loss row: widths of exactly one chunk, one
    chunk + 1, a partial second chunk and two full chunks (``max(lo, c0)`` / ``min(hi, c0 + n)`` clipping, ``dup[x - c0]``),
    at a small height."""
    maps, flow = loss_inputs(9600 + wl, 2, 2, 7, 6, wl)
    check_loss('h=6 W=%d' % wl, maps, flow)


def test_loss_flow_h_600_through_device_flow_losses():
    """flow_loss_rows_kernel at a true flow_h = 600 (loss rows of 1200: two chunks) through device_flow_losses and
    autograd, B = 1, three pairs."""
    L, h = 3, 600
    maps, flow = loss_inputs(9650, 1, L, 7, h, 2 * h)
    wv, wd = loss_ref(maps, flow, WEIGHTS)
    md = dev(maps).requires_grad_(True)
    got = tt.device_flow_losses(md, dev(flow), types.SimpleNamespace(flow_h=h, mm_th=MM_TH, seq_len=L + 1), L)
    sum(wt * t for wt, t in zip(WEIGHTS, got)).backward()
    g, dm = np.array([t.item() for t in got]), md.grad.cpu().numpy()
    gerr = float(np.max(np.abs(dm - wd)) / np.max(np.abs(wd)))
    print('loss flow_h=600: terms rel %s, dmaps max|d| / max|g| %.2e' % (np.abs(g / wv - 1), gerr))
    np.testing.assert_allclose(g, wv, rtol=1e-5, atol=0)
    assert gerr <= 1e-5
    assert np.all(dm[:, 0] == 0)


def loss_sizes(w):
    """(tag, h, W) of an up-sampling, an identity and a down-sampling loss size of a 2w x 4w map.  w = 1 has no height
    in [2, 2w), so its down-sampling case keeps h = 2 and shrinks the width (3 < 4w).  'wide': rows of about 300 columns, so
    that every map column is touched by more loss columns (about 2 W / 4w) than the row kernel has slices (nsub = 256 / 4w,
    4 .. 64) and no slice of a thread stays empty."""
    down = (2, 3) if w == 1 else (max(2, 2 * w - 3), 4 * w - 5)
    return (('up', 5 * w + 3, 9 * w + 5), ('identity', 2 * w, 4 * w), ('down',) + down, ('wide', 9, 301 + w))


@pytest.mark.parametrize('w', [1, 2, 5, 7, 16])
def test_loss_face_sizes_and_scales(w):
    """flow_loss_* at any face size: ``nsub = 256 / mw`` slices (all of them filled by the 'wide' size) and inactive
    threads (w = 5: 240 of 256 threads, w = 7 the control), w = 16 (the LDS map arrays exactly full, nsub = 4), w = 1
    (nsub = 64); and ``up_tap`` / ``first_at_least`` / ``up_weight`` on identity and down-sampling axes (h <= 2w: source
    indices skipped, i0 clamped) besides up-sampling."""
    for k, (tag, h, wl) in enumerate(loss_sizes(w)):
        assert (tag == 'up' and h > 2 * w and wl > 4 * w) or (tag == 'identity' and (h, wl) == (2 * w, 4 * w)) \
            or (tag == 'down' and h <= 2 * w and wl < 4 * w and h >= 2) or (tag == 'wide' and 2 * wl // (4 * w) >= 256 // (4 * w))
        maps, flow = loss_inputs(9700 + 10 * w + k, 2, 3, w, h, wl)
        check_loss('w=%d %s %dx%d' % (w, tag, h, wl), maps, flow)


def test_loss_face_17_is_refused():
    """w = 17 does not fit the LDS map arrays: ``_flow_loss_geometry`` raises instead of launching."""
    maps = torch.zeros(1, 2, 34, 68, device=DEV)
    flow = torch.zeros(1, 1, 40, 80, 2, device=DEV)
    with pytest.raises(ValueError, match='unsupported geometry'):
        ops.flow_loss_forward(maps, flow, MM_TH)
    with pytest.raises(ValueError, match='unsupported geometry'):
        ops.flow_loss_backward(maps, flow, torch.ones(3, device=DEV), MM_TH)


def test_loss_gradient_term_by_term():
    """flow_loss_rows_kernel, the three terms' gradients one at a time: one-hot upstream weights (1,0,0), (0,1,0), (0,0,1)
    against autograd of that term alone (a swap of g_t and g_m, or a mask term carrying 1 % of the signal, cannot hide),
    and ``loss_sm.backward()`` alone through DeviceFlowLoss (the other two upstream gradients arrive undefined: ``z(g)``).
    Map 0 of each clip stays exactly zero in all of them."""
    B, L, w, h, wl = 2, 3, 7, 40, 90
    maps, flow = loss_inputs(9800, B, L, w, h, wl)
    md, fd = dev(maps), dev(flow)
    refs = []
    for k in range(3):
        one = tuple(1.0 if j == k else 0.0 for j in range(3))
        _, wd = loss_ref(maps, flow, one)
        refs.append(wd)
        dm = ops.flow_loss_backward(md, fd, dev(np.float32(one)), MM_TH).cpu().numpy()
        err = float(np.max(np.abs(dm - wd)) / np.max(np.abs(wd)))
        print('loss term %d alone: dmaps max|d| / max|g| %.2e (max|g| %.3e)' % (k, err, np.max(np.abs(wd))))
        assert np.max(np.abs(wd)) > 0 and err <= 1e-5, (k, err)
        assert np.all(dm[:, 0] == 0)
    # the three gradients are different functions: a permutation of the weights is visible at the bound
    assert all(rel(refs[a], refs[b]) > 1e-2 for a, b in ((0, 1), (0, 2), (1, 2)))
    for k in range(3):
        m = dev(maps).requires_grad_(True)
        tt.device_flow_losses(m, fd, types.SimpleNamespace(mm_th=MM_TH), L)[k].backward()
        dm = m.grad.cpu().numpy()
        err = float(np.max(np.abs(dm - refs[k])) / np.max(np.abs(refs[k])))
        assert err <= 1e-5 and np.all(dm[:, 0] == 0), (k, err)


# ============================================================================= K5f: flow resize
def test_resize_grid_stride_second_pass():
    """flow_resize_kernel, grid-stride second pass: 40 flows of 240 x 480 to 480 x 960 are 18.4 M outputs, more than the
    65536 * 256 threads of the capped grid; every flow is compared in full (the float64 restatement runs flow by flow)."""
    F_, hi, wi, ho, wo = 40, 240, 480, 480, 960
    assert F_ * ho * wo > 65536 * 256
    flow = hashrng.normal(9900, (F_, hi, wi, 2), 0, 2.0)
    got = tt.resize_flow(dev(flow), ho).cpu().numpy()
    assert got.shape == (F_, ho, wo, 2)
    scale = np.max(np.abs(flow))
    err = [float(np.max(np.abs(got[f] - fr.resize_flow(flow[f], ho))) / scale) for f in range(F_)]
    print('resize 40 x (240x480 -> 480x960): max|d| / max|flow| = %.2e (second pass: %.2e)' % (max(err), max(err[36:])))
    assert max(err) <= 3e-7, err


TINY = [((1, 1), (1, 1)), ((1, 1), (5, 9)), ((2, 3), (7, 13)), ((3, 2), (7, 13)), ((3, 2), (2, 5)), ((1, 5), (28, 56)),
        ((2, 3), (28, 56)), ((3, 3), (1, 1)), ((8, 16), (28, 56)), ((8, 16), (5, 3)), ((2, 2), (8, 16))]


@pytest.mark.parametrize('hw_in,hw_out', TINY)
def test_resize_tiny_inputs(hw_in, hw_out):
    """flow_resize_kernel on inputs of 1 to 3 pixels per axis (every tap clamped: replicate on both sides at once) up to
    8 x 16, to larger and to smaller sizes, through ops.flow_resize with a scale; equal sizes: the scale alone, bit for bit."""
    flow = hashrng.normal(9950 + 17 * hw_in[0] + hw_in[1] + hw_out[0], (3,) + hw_in + (2,), 0, 2.0)
    fscale = 0.3125
    got = ops.flow_resize(dev(flow), hw_out[0], hw_out[1], fscale).cpu().numpy()
    want = fr.resize(flow, *hw_out) * fscale
    assert got.shape == want.shape
    err = float(np.max(np.abs(got - want)) / np.max(np.abs(flow)))
    print('resize %s -> %s: max|d| / max|flow| = %.2e' % (hw_in, hw_out, err))
    assert err <= 3e-7
    if hw_in == hw_out:
        np.testing.assert_array_equal(got, np.float32(fscale) * flow)


# ============================================================================= K5t: gates
def gates_ref(pre, bias, c_prev, dh, dc, round_dg=False):
    """float64: the slabs' sum + bias -> gates, c, h and the backward of sum(h dh + c dc) onto the pre-activations / c_prev."""
    g = (torch.from_numpy(pre).double().sum(0) + torch.from_numpy(bias).double()).requires_grad_(True)
    cp = torch.from_numpy(c_prev).double().requires_grad_(True)
    i, f, o, gg = g.chunk(4, 1)
    acts = torch.cat((torch.sigmoid(i), torch.sigmoid(f), torch.sigmoid(o), torch.tanh(gg)), 1)
    c = torch.sigmoid(f) * cp + torch.sigmoid(i) * torch.tanh(gg)
    h = torch.sigmoid(o) * torch.tanh(c)
    (h * torch.from_numpy(dh).double() + c * torch.from_numpy(dc).double()).sum().backward()
    return (h.detach().numpy(), c.detach().numpy(), acts.detach().numpy(), g.grad.numpy(), cp.grad.numpy())


def run_gates(seed, M, hc, splits, h_dtype, dg_dtype, ld_h, h_coff, pre_std=1.5):
    pre = hashrng.normal(seed, (splits, M, 4 * hc), 0, pre_std / splits ** 0.5)
    bias = hashrng.normal(seed + 1, (4 * hc,), 0, 0.3)
    c_prev = hashrng.normal(seed + 2, (M, hc))
    dh, dc = hashrng.normal(seed + 3, (M, hc)), hashrng.normal(seed + 4, (M, hc))
    h, c, acts, dg, dcp = gates_ref(pre, bias, c_prev, dh, dc)
    SENT = -77.0
    c_next = torch.empty(M, hc, device=DEV)
    h_f32 = torch.empty(M, hc, device=DEV)
    h_out = torch.full((M, ld_h), SENT, dtype=h_dtype, device=DEV)
    a_d = torch.empty(M, 4 * hc, device=DEV)
    ops.train_gates(dev(pre), splits, dev(bias), dev(c_prev), c_next, h_out, h_coff, h_f32, a_d, M, hc)
    ho = h_out.float().cpu().numpy()
    res = {'h': rel(h_f32.cpu().numpy(), h), 'c': rel(c_next.cpu().numpy(), c), 'acts': rel(a_d.cpu().numpy(), acts)}
    assert np.all(ho[:, :h_coff] == SENT) and np.all(ho[:, h_coff + hc:] == SENT)       # outside the window: untouched
    win = ho[:, h_coff:h_coff + hc]
    if h_dtype == torch.float32:
        assert np.array_equal(win, h_f32.cpu().numpy())
    else:
        res['h_bf16'] = close_bf16(win, h, 1e-6)
    dc_d = dev(dc)
    dg_d = torch.empty(M, 4 * hc, dtype=dg_dtype, device=DEV)
    ops.train_gates_backward(dev(dh), dc_d, a_d, dev(c_prev), c_next, dg_d, M, hc)
    if dg_dtype == torch.float32:
        res['dg'] = rel(dg_d.cpu().numpy(), dg)
    else:
        res['dg_bf16'] = close_bf16(dg_d.float().cpu().numpy(), dg, 1e-5)
    res['dc'] = rel(dc_d.cpu().numpy(), dcp)
    return res


def assert_gates(tag, res):
    print('gates %s: %s' % (tag, {k: '%.2e' % v for k, v in res.items()}))
    assert res['h'] <= 1e-6 and res['c'] <= 1e-6 and res['acts'] <= 1e-6, res
    assert res.get('h_bf16', 0) <= 1 and res.get('dg_bf16', 0) <= 1, res
    assert res.get('dg', 0) <= 1e-5 and res['dc'] <= 1e-5, res


def test_gates_splits_3():
    """train_gates_kernel with ``splits`` = 3: the reference sums the three slabs (and the bias) in float64; f32 h_out at
    h_coff > 0 in a wider row, sentinel outside.  Then train_gates_bwd_kernel (f32), d c_prev in place."""
    assert_gates('splits=3 f32', run_gates(10100, 12 * 49, 24, 3, torch.float32, torch.float32, 24 + 24 + 8, 24))


def test_gates_bf16_outputs():
    """train_gates_kernel with bf16 ``h_out`` (h_coff > 0, ld_h > h_coff + Hc: the columns outside the written window keep
    a sentinel) and train_gates_bwd_kernel with bf16 ``dgates`` at small size: one bf16 rounding of the float64 value
    (2^-8 relative) plus the f32 bound of the same quantity (1e-6 / 1e-5 of max), elementwise.  Hc = 25 is odd, so rows of
    bf16 elements start on 2-byte boundaries."""
    assert_gates('bf16 splits=2', run_gates(10200, 6 * 49, 25, 2, torch.bfloat16, torch.bfloat16, 25 + 17 + 9, 17))


def test_gates_grid_stride_second_pass():
    """train_gates_kernel and train_gates_bwd_kernel, grid-stride second pass: M * Hc = 1176 * 900 is just above the
    4096 * 256 threads of the capped grid (training reaches it from B = 4 at Hc = 1000); EVERY element of h, c, the four
    activations, dgates and d c_prev is compared, so an error in the stride cannot hide.  f32 and bf16 outputs."""
    M, hc = 6 * 49 * 4, 900
    assert 4096 * 256 < M * hc < 4096 * 256 + 16384
    assert_gates('large f32', run_gates(10300, M, hc, 1, torch.float32, torch.float32, hc, 0))
    assert_gates('large bf16', run_gates(10310, M, hc, 1, torch.bfloat16, torch.bfloat16, hc + 4, 4))


# ============================================================================= K5t: dgrad, CubePad adjoint, wgrad
def conv_pad64(x, w, b=None):
    return F.conv2d(cubepad_t(x, 1), w, b)


@pytest.mark.parametrize('n', [16, 72, 136])
@pytest.mark.parametrize('c_out', [8, 24, 40])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_dgrad_k_tails_and_n_tiles(dtype, c_out, n):
    """train_gemm_kernel<*, DGRAD> with ``9 * c_out % 32 != 0`` (K = 72, 216, 360: the ``kok`` tail, and K steps that
    straddle two taps) in f32 and bf16, ``n`` = 16, 72 (> 64, second N tile partial) and 136 (three tiles), ci0 > 0, faces
    1, 2, 3, 7 with 6 and 12 images (M tiles partial).  dxpad -> cubepad_adjoint (f32 dx, no mask) against float64 autograd
    of CubePad(1) + conv on the operands the kernel reads (bf16-rounded for bf16): only f32 accumulation remains, 1e-5."""
    ci0 = 5
    c_in = ci0 + n + 3
    for k, (face, n6) in enumerate(((1, 12), (2, 6), (3, 12), (7, 6))):
        seed = 10400 + 1000 * (dtype == torch.bfloat16) + 100 * k + c_out + n
        rnd = rb if dtype == torch.bfloat16 else (lambda t: t)
        w = rnd(torch.from_numpy(hashrng.normal(seed, (c_out, c_in, 3, 3), 0, (2.0 / (9 * c_in)) ** 0.5)))
        dy = rnd(torch.from_numpy(hashrng.normal(seed + 1, (n6, c_out, face, face))))
        x = torch.zeros(n6, c_in, face, face, dtype=torch.float64, requires_grad=True)
        (conv_pad64(x, w.double()) * dy.double()).sum().backward()
        want = x.grad[:, ci0:ci0 + n].permute(0, 2, 3, 1).numpy()
        pack = ops.DgradPack(dev(w), ci0, n, dtype)
        off, ent = ops.cubepad_inverse(face)
        out = torch.empty((n6, face, face, n), device=DEV)
        ops.cubepad_adjoint(pack.dgrad(ops.nchw_to_nhwc(dev(dy), out_dtype=dtype)), dev(off), dev(ent), out)
        err = rel(out.cpu().numpy(), want)
        print('dgrad %s c_out=%d n=%d face=%d n6=%d: rel %.2e' % (dtype, c_out, n, face, n6, err))
        assert np.max(np.abs(want)) > 0.1 and err <= 1e-5, (face, n6, err)


def relu_operand(seed, shape):
    """Normals pushed 0.01 away from zero, with about 15 % exact +0 and 15 % exact -0 (the ReLU mask is ``> 0``)."""
    a = hashrng.normal(seed, shape)
    a = a + np.copysign(np.float32(0.01), a)
    u = hashrng.uniform(seed + 1, shape)
    a = np.where(u < 0.15, np.float32(0.0), np.where(u < 0.3, np.float32(-0.0), a)).astype(np.float32)
    return a


@pytest.mark.parametrize('face', [2, 7])
@pytest.mark.parametrize('act_dtype,dx_dtype', [(torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16),
                                                (torch.float32, torch.bfloat16)])
def test_cubepad_adjoint_accumulate_mask_window_and_types(act_dtype, dx_dtype, face):
    """cubepad_adjoint_kernel: ``accumulate = 1`` onto a prefilled dx in f32 and in bf16 (the bf16 read-add-round is the
    contract: reference = round(bf16(dx) + sum)), ``act`` wider than n read at ``act_coff > 0`` (act_ld > n), f32 ``act``
    with bf16 ``dx``, and ``act`` holding exact zeros and negative zeros (mask is ``> 0``).  Reference: float64 autograd of
    the oracle's index-gather CubePad.  Also the plain write (accumulate = 0) over a sentinel-filled dx."""
    n6, n, act_coff, act_ld = 12, 20, 7, 33
    seed = 10600 + 10 * face + (act_dtype == torch.bfloat16) + 2 * (dx_dtype == torch.bfloat16)
    dxpad = hashrng.normal(seed, (n6, face + 2, face + 2, n))
    act = relu_operand(seed + 1, (n6, face, face, act_ld))
    act_t = torch.from_numpy(act).to(act_dtype)
    a64 = act_t.double().numpy()
    assert np.all((a64 == 0) | (np.abs(a64) >= 1e-3))              # the ReLU decision is not on the knife edge
    win = a64[..., act_coff:act_coff + n]
    assert np.any(np.signbit(win) & (win == 0)) and np.any(~np.signbit(win) & (win == 0)) and np.any(win > 0) and np.any(win < 0)
    assert np.mean((win > 0) != (a64[..., :n] > 0)) > 0.2          # reading at column 0 instead would be visible
    x = torch.zeros(n6, n, face, face, dtype=torch.float64, requires_grad=True)
    (cubepad_t(x, 1) * torch.from_numpy(dxpad).double().permute(0, 3, 1, 2)).sum().backward()
    s = np.where(win > 0, x.grad.permute(0, 2, 3, 1).numpy(), 0.0)
    pre = torch.from_numpy(hashrng.normal(seed + 3, (n6, face, face, n), 0, 2.0)).to(dx_dtype)
    off, ent = ops.cubepad_inverse(face)
    off, ent = dev(off), dev(ent)
    for accumulate in (False, True):
        dx = pre.clone().to(DEV)
        ops.cubepad_adjoint(dev(dxpad), off, ent, dx, act=act_t.to(DEV), act_coff=act_coff, accumulate=accumulate)
        want = s + pre.double().numpy() if accumulate else s
        got = dx.float().cpu().numpy()
        if dx_dtype == torch.float32:
            err = rel(got, want)
            assert err <= 1e-5, (accumulate, err)
        else:
            err = close_bf16(got, want, 1e-5)
            assert err <= 1, (accumulate, err)
        print('adjoint face=%d act=%s dx=%s accumulate=%d: %.2e' % (face, act_dtype, dx_dtype, accumulate, err))
        assert np.all(got[win <= 0] == (pre.float().numpy()[win <= 0] if accumulate else 0.0))   # masked: nothing added


def wgrad_ref(x, dy, c_in, c_out):
    """float64 dW, db of CubePad(1) + 3x3 conv: x [n6, ld, f, f] (channels [0, c_in) used), dy [n6, c_out, f, f]."""
    w = torch.zeros(c_out, c_in, 3, 3, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(c_out, dtype=torch.float64, requires_grad=True)
    (conv_pad64(x.double()[:, :c_in], w, b) * dy.double()).sum().backward()
    return w.grad.numpy(), b.grad.numpy()


def wgrad_inputs(seed, n6, face, ld, c_out, dtype):
    rnd = rb if dtype == torch.bfloat16 else (lambda t: t)
    x = rnd(torch.from_numpy(hashrng.normal(seed, (n6, ld, face, face))))
    dy = rnd(torch.from_numpy(hashrng.normal(seed + 1, (n6, c_out, face, face))))
    to = lambda t: ops.nchw_to_nhwc(dev(t), out_dtype=dtype)
    return x, dy, to(x), to(dy), dev(ops.cubepad_table(face, 1))


@pytest.mark.parametrize('c_in', [7, 64, 10])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_wgrad_bias_column_faces_and_no_bias(dtype, c_in):
    """train_gemm_kernel<*, WGRAD>: ``c_in`` chosen by where the bias column 9 c_in of the GEMM falls in its 64-wide N tile
    (7: N = 64, the last column of the only tile; 64: alone in a tile of its own; 10: mid-tile), ``ldx > c_in``, c_out = 72
    (two M tiles, the second partial), faces 1, 2, 3 (the table's corner entries) besides 7; and ``db = None`` (N = 9 c_in,
    no ones column): dw bit-equal to the run with db.  float64 autograd on the operands the kernel reads: 1e-5 of max."""
    c_out, ld = 72, c_in + 3
    for k, (face, n6) in enumerate(((1, 24), (2, 12), (3, 6), (7, 12))):
        seed = 10800 + 1000 * (dtype == torch.bfloat16) + 100 * k + c_in
        x, dy, xd, dyd, tab = wgrad_inputs(seed, n6, face, ld, c_out, dtype)
        ww, wb = wgrad_ref(x, dy, c_in, c_out)
        dw = torch.full((c_out, c_in, 3, 3), 55.0, device=DEV)
        db = torch.full((c_out,), 55.0, device=DEV)
        ops.conv_wgrad(dyd, xd, c_in, tab, dw, db)
        e = (rel(dw.cpu().numpy(), ww), rel(db.cpu().numpy(), wb))
        print('wgrad %s c_in=%d face=%d n6=%d: rel %.2e / %.2e' % (dtype, c_in, face, n6, e[0], e[1]))
        assert np.max(np.abs(ww)) > 1 and np.max(np.abs(wb)) > 1
        assert e[0] <= 1e-5 and e[1] <= 1e-5, (face, e)
        dw2 = torch.full((c_out, c_in, 3, 3), -55.0, device=DEV)
        ops.conv_wgrad(dyd, xd, c_in, tab, dw2, None)
        assert torch.equal(dw2, dw)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_wgrad_accumulate(dtype):
    """train_gemm_kernel<*, WGRAD> with ``accumulate = 1``: a launch on the first half of the steps followed by an
    accumulating launch on the second half equals the float64 gradient over all steps; dw and db prefilled with a known
    tensor are added to, not overwritten; with ``db = None`` an accumulating launch adds to dw alone."""
    n6, face, c_in, ld, c_out = 24, 7, 10, 12, 72
    x, dy, xd, dyd, tab = wgrad_inputs(11000 + (dtype == torch.bfloat16), n6, face, ld, c_out, dtype)
    ww, wb = wgrad_ref(x, dy, c_in, c_out)
    dw = torch.full((c_out, c_in, 3, 3), 55.0, device=DEV)
    db = torch.full((c_out,), 55.0, device=DEV)
    ops.conv_wgrad(dyd[:12], xd[:12], c_in, tab, dw, db)
    ops.conv_wgrad(dyd[12:], xd[12:], c_in, tab, dw, db, accumulate=True)
    e = (rel(dw.cpu().numpy(), ww), rel(db.cpu().numpy(), wb))
    print('wgrad accumulate %s: halves rel %.2e / %.2e' % (dtype, e[0], e[1]))
    assert e[0] <= 1e-5 and e[1] <= 1e-5, e
    pw, pb = hashrng.normal(11010, (c_out, c_in, 3, 3), 0, 30.0), hashrng.normal(11011, (c_out,), 0, 30.0)
    dw, db = dev(pw), dev(pb)
    ops.conv_wgrad(dyd, xd, c_in, tab, dw, db, accumulate=True)
    e = (rel(dw.cpu().numpy(), ww + pw), rel(db.cpu().numpy(), wb + pb))
    print('wgrad accumulate %s: prefilled rel %.2e / %.2e' % (dtype, e[0], e[1]))
    assert e[0] <= 1e-5 and e[1] <= 1e-5, e
    assert rel(ww + pw, ww) > 0.1 and rel(ww + pw, pw.astype(np.float64)) > 0.1      # neither operand alone passes
    dw2 = dev(pw)
    ops.conv_wgrad(dyd, xd, c_in, tab, dw2, None, accumulate=True)
    assert torch.equal(dw2, dw)


# ============================================================================= K5t: saliency
def sal_tables(w):
    """(face_map int64 [8 w^2], sampling positions f32 [8 w^2, 2]) of the CPU reference: the oracle's cube -> equirectangular
    tables.  At w = 1 the reference's own mapping is 0 / 0 (cube coordinates in [0, w - 1] normalised by their maximum), so
    there the kernels get a synthetic table instead: a hashed face per pixel and positions in [-0.95, 0.95], whose four taps
    straddle the single pixel (zero padding outside)."""
    if w == 1:
        return (hashrng.integers(11100, (8,), 0, 6), hashrng.uniform(11101, (8, 2), -0.95, 0.95))
    fm, coord = o_c2e.c2e_tables(w)
    return fm.reshape(-1).astype(np.int64), o_c2e.sample_pixel_coords(coord, w).reshape(-1, 2)


def sal_ref(h, w, fm, pc):
    """float64 to_equi_nn of h [6B, C, w, w] (bilinear taps with f32 weights as ``ref_map`` of tests/test_train_gpu.py, zero
    padding): the sampled planes [B, 8 w^2, C], differentiable."""
    x0, y0 = np.floor(pc[:, 0]), np.floor(pc[:, 1])
    fx, fy = (pc[:, 0] - x0).astype(np.float32), (pc[:, 1] - y0).astype(np.float32)
    idx, wts = [], []
    for k, wt in enumerate(((1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy)):
        xx, yy = x0.astype(np.int64) + (k & 1), y0.astype(np.int64) + (k >> 1)
        ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < w)
        idx.append(torch.from_numpy((fm * w + np.clip(yy, 0, w - 1)) * w + np.clip(xx, 0, w - 1)))
        wts.append(torch.from_numpy(np.where(ok, wt, 0).astype(np.float64)))
    out = []
    for b in range(h.shape[0] // 6):
        flat = h[6 * b:6 * b + 6].permute(0, 2, 3, 1).reshape(6 * w * w, -1)
        out.append(sum(flat[idx[k]] * wts[k][:, None] for k in range(4)))
    return torch.stack(out)


def check_saliency(tag, h_np, w, seed, ties):
    """ops.saliency_forward / backward against sal_ref: map 1e-5 absolute, argmax EQUAL to torch.max's on the CPU, dh (added
    onto a prefilled tensor) 1e-5 of max.  Asserts first that every pixel's maximum is either exactly tied or at least
    1e-4 above every other channel."""
    n6, C = h_np.shape[0], h_np.shape[1]
    B = n6 // 6
    h = torch.from_numpy(h_np).double().requires_grad_(True)
    fm, pc = sal_tables(w)
    planes = sal_ref(h, w, fm, pc)
    mx, am = planes.max(dim=2)
    p = planes.detach().numpy()
    near = p >= p.max(axis=2, keepdims=True) - 1e-4
    exact = p == p.max(axis=2, keepdims=True)
    assert np.array_equal(near, exact)                              # a gap of 1e-4, or an exact tie
    assert np.array_equal(am.numpy(), np.argmax(exact, axis=2))     # torch.max on the CPU takes the lowest tied channel
    if ties is None:
        assert np.all(exact.sum(2) == 1)
    else:
        assert np.mean(exact.sum(2) >= ties) > 0.9
    dmap = hashrng.normal(seed + 50, (B, 2 * w, 4 * w))
    (mx.view(B, 2 * w, 4 * w) * torch.from_numpy(dmap).double()).sum().backward()
    if w == 1:
        fm_d, pc_d = dev(fm.astype(np.int8).reshape(2, 4)), dev(pc.reshape(2, 4, 2))
    else:
        fm_d, pc_d = Cube2Equi(w, device=torch.device(DEV))._tables()       # the package's own tables against the oracle's
    eo, ee = ops.c2e_inverse(fm_d.cpu().numpy(), pc_d.cpu().numpy(), w)
    hd = ops.nchw_to_nhwc(dev(h_np))
    mx_d = torch.empty(B, 2 * w, 4 * w, device=DEV)
    am_d = torch.full((B, 2 * w, 4 * w), -1, dtype=torch.int32, device=DEV)
    ops.saliency_forward(hd, fm_d, pc_d, mx_d, am_d)
    merr = float(np.max(np.abs(mx_d.cpu().numpy().reshape(B, -1) - mx.detach().numpy())))
    wrong = int(np.sum(am_d.cpu().numpy().reshape(B, -1) != am.numpy()))
    pre = hashrng.normal(seed + 51, (n6, w, w, C))
    dh = dev(pre)
    ops.saliency_backward(dev(dmap), am_d, pc_d, dev(eo), dev(ee), dh)
    want = pre + h.grad.permute(0, 2, 3, 1).numpy()
    derr = rel(dh.cpu().numpy(), want)
    print('saliency %s: map max|d| %.2e, argmax mismatches %d, dh rel %.2e' % (tag, merr, wrong, derr))
    assert merr <= 1e-5
    assert wrong == 0
    assert derr <= 1e-5 and rel(want, pre.astype(np.float64)) > 0.1


@pytest.mark.parametrize('C', [1, 63, 65, 100])
@pytest.mark.parametrize('w', [1, 2, 3, 7])
def test_saliency_faces_and_channel_counts(w, C):
    """sal_forward_kernel / sal_backward_kernel at ``w`` = 1, 2, 3 besides 7 and ``C`` = 1, 63, 65, 100 (a partial wave,
    one channel past a wave, a partial second round of the lane loop), B = 3: map, the ``argmax`` output itself, and dh
    added onto a prefilled tensor, against float64 autograd."""
    seed = 11200 + 100 * w + C                       # the first seed tried meets the gap condition at every (w, C)
    check_saliency('w=%d C=%d' % (w, C), hashrng.normal(seed, (18, C, w, w)), w, seed, None)


@pytest.mark.parametrize('w', [2, 7])
@pytest.mark.parametrize('case', ['same_lane', 'other_lane', 'three', 'all_equal', 'all_zero'])
def test_saliency_exact_ties(case, w):
    """sal_forward_kernel, exact ties between channels: the lowest channel must win, as torch.max on the CPU.  Duplicate
    (bit-identical) channel planes raised above the rest (values below 10, so the absolute 1e-5 of the map holds): (a) in
    the same lane (c and c + 64: the strict ``>`` of the lane loop), (b) in different lanes, the higher channel in the lower
    lane (the ``oi < bi`` rule of the wave reduction), three planes across both, every channel the same plane, and an
    all-zero h.  ``argmax`` is compared directly."""
    C, seed = 100, 11900 + w
    h = hashrng.normal(seed, (18, C, w, w))
    if case == 'all_zero':
        h[:] = 0
    elif case == 'all_equal':
        h[:] = np.abs(h[:, 40:41]) + 5.0
    else:
        dup = {'same_lane': (3, 67), 'other_lane': (70, 9), 'three': (69, 5, 38)}[case]
        top = np.abs(h[:, dup[0]]) + 5.0            # above every other channel (|normal| < 4.3) under any tap weights
        for c in dup:
            h[:, c] = top
    ties = {'same_lane': 2, 'other_lane': 2, 'three': 3}.get(case, C)
    check_saliency('ties %s w=%d' % (case, w), h, w, seed, ties)
