"""CPU tests of the flow resize and flow loss (include/cp360.h "K5f", csrc/flow_loss.hip): the numpy restatement of the
cv2 INTER_CUBIC resize (tests/flow_restate.py) and its known answers, the library's host tables against it, and the new entry
points' declarations and argument checks (no launch)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cp_360_weakly_supervised_saliency_amd import _lib, ops
from cp_360_weakly_supervised_saliency_amd.utils import hashrng
from tests import flow_restate as fr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOW_SYMBOLS = ['cp360_flow_resize_coeffs_host', 'cp360_flow_resize', 'cp360_flow_loss_work_bytes', 'cp360_flow_loss_forward',
                'cp360_flow_loss_backward']


def test_restatement_downscale_taps():
    """A 2x downscale samples halfway between two source pixels: f = 0.5, taps (-0.09375, 0.59375, 0.59375, -0.09375)."""
    ofs, coef = fr.cubic_tables(480, 240)
    np.testing.assert_array_equal(ofs, 2 * np.arange(240))
    np.testing.assert_array_equal(coef, np.tile(np.float32([-0.09375, 0.59375, 0.59375, -0.09375]), (240, 1)))


def test_restatement_identity_and_constant():
    ofs, coef = fr.cubic_tables(56, 56)
    np.testing.assert_array_equal(ofs, np.arange(56))
    np.testing.assert_array_equal(coef, np.tile(np.float32([0, 1, 0, 0]), (56, 1)))
    flow = hashrng.normal(9500, (2, 28, 56, 2))
    np.testing.assert_array_equal(fr.resize(flow, 28, 56), flow.astype(np.float64))
    for hw_in, hw_out in (((480, 960), (240, 480)), ((240, 480), (480, 960)), ((480, 640), (240, 480)), ((30, 60), (28, 56))):
        const = np.broadcast_to(np.float32([1.25, -3.5]), hw_in + (2,))
        out = fr.resize(const, *hw_out)
        assert out.shape == hw_out + (2,)
        np.testing.assert_allclose(out, np.broadcast_to([1.25, -3.5], out.shape), rtol=0, atol=4e-7)


def test_restatement_replicates_borders():
    """Upscaling: the first output's taps start left of the image and read pixel 0 (replicate), the last output's run past the
    right edge and read pixel n - 1: a spike in a border pixel collects the weights of every clamped tap."""
    ofs, coef = fr.cubic_tables(4, 8)
    assert ofs[0] == -1 and ofs[-1] == 3
    img = np.zeros((1, 4, 2))
    img[0, 0, 0] = 1.0
    out = fr.resize(img, 1, 8)
    want0 = coef[0, 0] + coef[0, 1] + coef[0, 2]                      # taps -2, -1, 0 -> pixel 0; tap 1 -> pixel 1
    np.testing.assert_allclose(out[0, 0, 0], want0, rtol=1e-7)
    assert out[0, 0, 1] == 0.0
    right = np.zeros((1, 4, 2))
    right[0, 3, 0] = 1.0
    out = fr.resize(right, 1, 8)
    np.testing.assert_allclose(out[0, 7, 0], coef[7, 1] + coef[7, 2] + coef[7, 3], rtol=1e-7)   # taps 3, 4, 5 -> pixel 3


def test_restatement_scale_divides_by_width():
    flow = np.ones((1, 480, 960, 2), np.float32)
    np.testing.assert_allclose(fr.resize_flow(flow, 240), 0.25, rtol=1e-6)
    np.testing.assert_allclose(fr.resize_flow(flow, 480), 0.5, rtol=0)


@pytest.mark.parametrize('n_in,n_out', [(480, 240), (960, 480), (480, 28), (240, 480), (640, 480), (56, 56),
                                        # inputs of 1 to 3 pixels (every tap clamped) up to 8 and 16, both directions
                                        (1, 1), (1, 7), (1, 28), (2, 5), (2, 13), (3, 2), (3, 7), (3, 56), (5, 3), (8, 28),
                                        (16, 56), (16, 3), (8, 1)])
def test_host_tables_equal_restatement(n_in, n_out):
    got_o, got_c = ops.flow_resize_coeffs(n_in, n_out)
    want_o, want_c = fr.cubic_tables(n_in, n_out)
    np.testing.assert_array_equal(got_o, want_o)
    np.testing.assert_array_equal(got_c.view(np.uint32), want_c.view(np.uint32))


def test_loss_restatement_equals_flow_losses():
    """tests/flow_restate.py ``loss_terms`` (any [H, W], already-scaled flow: the float64 reference of the GPU tests) gives
    the terms and the map gradient of ``flow_losses`` on a W = 2 H case, in float64, to rounding (1e-13)."""
    import types

    import torch

    from cp_360_weakly_supervised_saliency_amd.temporal_model import train_temporal as tt
    B, L, h, w = 2, 3, 20, 3
    maps = hashrng.uniform(9510, (B, L + 1, 2 * w, 4 * w), 0.0, 1.0, dtype=np.float64)
    n = hashrng.normal(9511, (B, L, h, 2 * h, 2), dtype=np.float64)
    u = hashrng.uniform(9512, (B, L, h, 2 * h, 1))
    scaled = n * np.where(u < 0.1, 6.0, 0.12)                   # both mask branches, some warps outside the image
    st = np.sqrt((scaled ** 2).sum(-1)) < 0.15
    assert 0.2 < st.mean() < 0.9
    res = []
    for fn in (lambda m: tt.flow_losses(m, torch.from_numpy(2.0 * scaled), types.SimpleNamespace(flow_h=h, mm_th=0.15, seq_len=L + 1), L),
               lambda m: fr.loss_terms(m, torch.from_numpy(scaled), 0.15)):
        m = torch.from_numpy(maps).requires_grad_(True)
        terms = fn(m)
        (0.7 * terms[0] + terms[1] + 0.01 * terms[2]).backward()
        res.append((np.array([t.item() for t in terms]), m.grad.numpy()))
    assert np.all(res[0][0] > 0)
    np.testing.assert_allclose(res[1][0], res[0][0], rtol=1e-13, atol=0)
    np.testing.assert_allclose(res[1][1], res[0][1], rtol=0, atol=1e-13 * np.max(np.abs(res[0][1])))
    assert np.all(res[1][1][:, 0] == 0) and np.max(np.abs(res[1][1][:, 1:])) > 0


def test_flow_entry_points_declared_and_bound():
    hdr = open(os.path.join(REPO, 'include', 'cp360.h')).read()
    assert hdr.index('K5t: ConvLSTM training') < hdr.index('K5w:') < hdr.index('K5f: flow resize and flow loss')
    sect = hdr[hdr.index('K5f: flow resize and flow loss'):hdr.index('K7:')]
    assert sorted(set(re.findall(r'\b(cp360_[a-z0-9_]+)\s*\(', sect))) == sorted(FLOW_SYMBOLS)
    assert set(FLOW_SYMBOLS) <= set(_lib.PUBLIC_SYMBOLS)
    L = _lib.lib()
    for name in FLOW_SYMBOLS:
        assert hasattr(L, name)
    assert L.cp360_version() == _lib.ABI_VERSION == 306


def test_flow_entry_points_validate_without_gpu():
    L = _lib.lib()
    one = C.c_void_p(16)
    buf = (C.c_int32 * 4)()
    assert L.cp360_flow_resize_coeffs_host(4, 8, None, buf) == -5
    assert L.cp360_flow_resize_coeffs_host(0, 8, buf, buf) == -1
    # resize: dtype, NULL, shape, missing tables for a real resize
    assert L.cp360_flow_resize(_lib.BF16, one, 1, 480, 960, one, 240, 480, one, one, one, one, 0.25, None) == -4
    assert L.cp360_flow_resize(_lib.F32, None, 1, 480, 960, one, 240, 480, one, one, one, one, 0.25, None) == -5
    assert L.cp360_flow_resize(_lib.F32, one, 0, 480, 960, one, 240, 480, one, one, one, one, 0.25, None) == -1
    assert L.cp360_flow_resize(_lib.F32, one, 1, 480, 960, one, 240, 480, None, one, one, one, 0.25, None) == -5
    # loss: work size, dtype, shape, face limit, NULL
    assert L.cp360_flow_loss_work_bytes(4, 3, 7, 480, 960) == 4 * max(12 * 225 * 3, 12 * 480 * 28)
    assert L.cp360_flow_loss_work_bytes(1, 3, 7, 28, 56) == 4 * max(3 * 1 * 3, 3 * 28 * 28)
    assert L.cp360_flow_loss_work_bytes(1, 3, 17, 28, 56) == 0
    assert L.cp360_flow_loss_forward(_lib.BF16, one, one, 1, 3, 7, 28, 56, 0.15, one, one, None) == -4
    assert L.cp360_flow_loss_forward(_lib.F32, one, one, 0, 3, 7, 28, 56, 0.15, one, one, None) == -1
    assert L.cp360_flow_loss_forward(_lib.F32, one, one, 1, 3, 7, 1, 56, 0.15, one, one, None) == -1
    assert L.cp360_flow_loss_forward(_lib.F32, one, one, 1, 3, 17, 28, 56, 0.15, one, one, None) == -8
    assert L.cp360_flow_loss_forward(_lib.F32, one, one, 1, 3, 7, 28, 56, 0.15, None, one, None) == -5
    assert L.cp360_flow_loss_backward(_lib.F16, one, one, one, 1, 3, 7, 28, 56, 0.15, one, one, None) == -4
    assert L.cp360_flow_loss_backward(_lib.F32, one, one, None, 1, 3, 7, 28, 56, 0.15, one, one, None) == -5
    assert L.cp360_flow_loss_backward(_lib.F32, one, one, one, 1, 0, 7, 28, 56, 0.15, one, one, None) == -1
