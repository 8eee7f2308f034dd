"""CPU tests of ConvLSTM training (temporal_model/train_temporal.py, data/dataset.py, include/cp360.h "K5t"): the flow loss
against the reference's own train() (tests/golden/clstm_train.npz, tests/golden/make_golden_train.py), the mesh grid, the
dataset's window list, and the new C entry points' declarations, host tables and argument checks (no launch)."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

from oracle import o_c2e, o_cubepad
from cp_360_weakly_supervised_saliency_amd import _lib, ops
from cp_360_weakly_supervised_saliency_amd.data.dataset import Sal360Dataset
from cp_360_weakly_supervised_saliency_amd.model.clstm import ConvLSTMCell
from cp_360_weakly_supervised_saliency_amd.model.clstm_train import ClstmTraining
from cp_360_weakly_supervised_saliency_amd.temporal_model import train_temporal as tt
from cp_360_weakly_supervised_saliency_amd.utils import hashrng

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, 'tests', 'golden', 'clstm_train.npz')
TRAIN_SYMBOLS = ['cp360_train_gates', 'cp360_train_gates_backward', 'cp360_train_dgrad_packed_bytes', 'cp360_train_dgrad_pack',
                 'cp360_train_dgrad', 'cp360_train_cubepad_inverse_host', 'cp360_train_cubepad_adjoint', 'cp360_train_wgrad',
                 'cp360_train_saliency_forward', 'cp360_train_c2e_inverse_host', 'cp360_train_saliency_backward']


def golden():
    g = np.load(GOLD)
    cfg = types.SimpleNamespace(**{str(k): float(v) for k, v in zip(g['cfg_keys'], g['cfg_vals'])})
    cfg.seq_len, cfg.flow_h = int(cfg.seq_len), int(cfg.flow_h)
    return g, cfg


def golden_batch(g, it):
    seq_seed, flow_seed, _, B, T, ch, w, fh, _ = (int(v) for v in g['seeds'])
    seq = [hashrng.uniform(seq_seed + 10 * it + t, (B, 6, ch, w, w), 0.0, 4.0) for t in range(T)]
    flow = [hashrng.normal(flow_seed + 10 * it + t, (B, fh, 2 * fh, 2), 0.0, 0.4) for t in range(T)]
    return seq, flow


def test_flow_loss_matches_reference_train():
    """train_step's torch part on the reference's own maps of iteration 1 gives the reference's three loss terms."""
    g, cfg = golden()
    _, flow = golden_batch(g, 0)
    flow = torch.from_numpy(np.stack(flow, 1))
    sm, tmp, mask = tt.flow_losses(torch.from_numpy(g['maps_it0']), flow, cfg, tmp_loss_len=3)
    got = np.array([sm.item(), tmp.item(), mask.item()])
    np.testing.assert_allclose(got, g['losses'][0], rtol=2e-5, atol=0)


def test_flow_must_be_at_loss_resolution():
    g, cfg = golden()
    maps = torch.from_numpy(g['maps_it0'])
    with pytest.raises(ValueError, match='loss resolution'):
        tt.flow_losses(maps, torch.zeros(2, 5, 28, 28, 2), cfg)
    with pytest.raises(ValueError, match='loss resolution'):
        tt.check_flow(torch.zeros(1, 5, 480, 640, 2), 480)


def test_generate_meshgrid():
    flow = torch.zeros(3, 28, 56, 2)
    m = tt.generate_meshgrid(flow)
    assert m.shape == (3, 2, 28, 56) and m.dtype == torch.float32
    xs = (np.arange(56) / 55.0 * 2 - 1).astype(np.float32)
    ys = (np.arange(28) / 27.0 * 2 - 1).astype(np.float32)
    np.testing.assert_allclose(m[1, 0].numpy(), np.broadcast_to(xs[None, :], (28, 56)), atol=1e-6)
    np.testing.assert_allclose(m[2, 1].numpy(), np.broadcast_to(ys[:, None], (28, 56)), atol=1e-6)
    assert m[0, 0, 0, 0] == -1 and m[0, 0, 0, -1] == 1 and m[0, 1, -1, 0] == 1


def test_batch_normalisation_spans_all_clips_and_frames():
    seq = torch.from_numpy(hashrng.uniform(7300, (2, 5, 6, 4, 3, 3), -2.0, 5.0))
    n = tt.normalize_batch(seq)
    assert float(n.min()) == 0.0 and float(n.max()) == 1.0
    mn = seq.min()
    np.testing.assert_array_equal(n.numpy(), ((seq - mn) / (seq - mn).max()).numpy())


def test_dataset_windows(tmp_path):
    """Sal360Dataset: the categories of the list, windows starting below max_len - seq_len + 1, (seq, motion, category,
    filename) items in sorted order (data/dataset.py:13-83 of the reference)."""
    vid, mot = tmp_path / 'vid', tmp_path / 'mot'
    for cat, n in (('b_cat', 8), ('a_cat', 7), ('skip', 9)):
        (vid / cat / 'cube_feat').mkdir(parents=True)
        (mot / cat / 'motion').mkdir(parents=True)
        for i in range(n):
            np.save(str(vid / cat / 'cube_feat' / ('%06d.npy' % i)), np.full((6, 2, 3, 3), 100 * len(cat) + i, np.float32))
            np.save(str(mot / cat / 'motion' / ('%06d.npy' % i)), np.full((4, 8, 2), -i, np.float32))
    lst = tmp_path / 'list.txt'
    lst.write_text('b_cat\na_cat\n')
    ds = Sal360Dataset(str(vid), str(mot), str(lst), 3)
    # max_len = 6 (a_cat) / 7 (b_cat): windows start at 0 .. 3 / 0 .. 4
    want = [('a_cat', i) for i in range(4)] + [('b_cat', i) for i in range(5)]
    assert len(ds) == len(want)
    assert [os.path.basename(p) for p in ds.data] == ['%06d.npy' % i for _, i in want]
    for k, (cat, i) in enumerate(want):
        seq, motion, category, filename = ds[k]
        assert category == cat and filename == '%06d.npy' % i
        assert len(seq) == len(motion) == 3
        assert [float(s[0, 0, 0, 0]) for s in seq] == [100 * len(cat) + i + o for o in range(3)]
        assert [float(m[0, 0, 0]) for m in motion] == [-(i + o) for o in range(3)]
        assert seq[0].dtype == torch.float32 and tuple(seq[0].shape) == (6, 2, 3, 3)


def test_train_entry_points_declared_and_bound():
    hdr = open(os.path.join(REPO, 'include', 'cp360.h')).read()
    sect = hdr[hdr.index('K5t: ConvLSTM training'):hdr.index('K5w:')]
    assert sorted(set(re.findall(r'\b(cp360_train_[a-z0-9_]+)\s*\(', sect))) == sorted(TRAIN_SYMBOLS)
    assert set(TRAIN_SYMBOLS) <= set(_lib.PUBLIC_SYMBOLS)
    L = _lib.lib()
    for name in TRAIN_SYMBOLS:
        assert hasattr(L, name)
    assert L.cp360_version() == _lib.ABI_VERSION == 306


def test_train_entry_points_validate_without_gpu():
    L = _lib.lib()
    one = C.c_void_p(16)
    assert L.cp360_train_dgrad_packed_bytes(_lib.F32, 4000, 1000) == 1000 * 9 * 4000 * 4
    assert L.cp360_train_dgrad_packed_bytes(_lib.BF16, 4000, 4000) == 4000 * 9 * 4000 * 2
    assert L.cp360_train_dgrad_packed_bytes(_lib.F16, 32, 8) == 0
    assert L.cp360_train_dgrad(_lib.F32, one, 5, 7, 32, one, 8, one, None) == -2          # not 6N faces
    assert L.cp360_train_dgrad(_lib.F32, None, 6, 7, 32, one, 8, one, None) == -5
    assert L.cp360_train_dgrad(_lib.F16, one, 6, 7, 32, one, 8, one, None) == -4          # fp16 training: no
    assert L.cp360_train_dgrad_pack(_lib.F32, one, 32, 16, 8, 9, one, None) == -1          # ci0 + n > c_in
    assert L.cp360_train_wgrad(_lib.BF16, one, one, 8, one, 12, 7, 32, 16, one, None, 0, None) == -1   # ldx < c_in
    assert L.cp360_train_wgrad(_lib.BF16, one, one, 16, one, 7, 7, 32, 16, one, None, 0, None) == -2
    assert L.cp360_train_wgrad(_lib.BF16, one, one, 16, None, 6, 7, 32, 16, one, None, 0, None) == -5
    assert L.cp360_train_gates(one, 1, one, one, one, one, _lib.F32, 8, 4, None, None, 294, 8, None) == -5   # no acts
    assert L.cp360_train_gates(one, 1, one, one, one, one, _lib.F32, 8, 4, None, one, 294, 8, None) == -1    # h_coff + Hc > ld
    assert L.cp360_train_gates_backward(one, one, one, one, one, one, _lib.F16, 294, 8, None) == -4
    assert L.cp360_train_cubepad_adjoint(one, one, one, 6, 7, 8, one, _lib.F32, 8, 4, one, _lib.F32, 0, None) == -1
    assert L.cp360_train_saliency_backward(one, one, one, one, None, one, 1, 8, 7, None) == -5


@pytest.mark.parametrize('face', [1, 2, 4, 7, 14])
def test_cubepad_inverse_table(face):
    """Every padded position of CubePad(1) appears once, under its source pixel, in ascending order (the gather order of
    the adjoint kernel)."""
    off, ent = ops.cubepad_inverse(face)
    tab = o_cubepad.cubepad_table(face, 1, 1, 1, 1).reshape(-1)
    assert off[0] == 0 and off[-1] == tab.size and np.all(np.diff(off) >= 1)
    assert sorted(ent.tolist()) == list(range(tab.size))
    for q in range(6 * face * face):
        e = ent[off[q]:off[q + 1]]
        assert np.all(tab[e] == q) and np.all(np.diff(e) > 0)


def test_c2e_inverse_table():
    """The (pixel, tap) pairs of to_equi_nn's bilinear sampling that land inside a face, grouped by the cube pixel they read."""
    w = 7
    fm, coord = o_c2e.c2e_tables(w)
    pc = o_c2e.sample_pixel_coords(coord, w)
    off, ent = ops.c2e_inverse(fm.astype(np.int8), pc, w)
    want = {}
    fmf, pcf = fm.reshape(-1), pc.reshape(-1, 2)
    for pix in range(8 * w * w):
        x0, y0 = int(np.floor(pcf[pix, 0])), int(np.floor(pcf[pix, 1]))
        for k in range(4):
            xx, yy = x0 + (k & 1), y0 + (k >> 1)
            if 0 <= xx < w and 0 <= yy < w:
                want.setdefault((fmf[pix] * w + yy) * w + xx, []).append(4 * pix + k)
    assert off[-1] == ent.size == sum(len(v) for v in want.values())
    for q in range(6 * w * w):
        assert ent[off[q]:off[q + 1]].tolist() == want.get(q, [])


def test_training_refuses_unsupported_configurations():
    with pytest.raises(ValueError, match='input_size == hidden_size'):
        ClstmTraining(ConvLSTMCell(8, 16))
    with pytest.raises(ValueError, match="'fp32' or 'bf16'"):
        ClstmTraining(ConvLSTMCell(8, 8, precision='fp16'))
