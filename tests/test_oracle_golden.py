"""Pin the oracle against fixtures produced by the reference itself
(tests/golden/make_golden.py).  CPU only."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from oracle import o_cubepad, o_e2c, o_c2e, o_resnet, o_clstm
from cp_360_weakly_supervised_saliency_amd.utils import hashrng, synth
from tests.golden import make_golden as mg


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ------------------------------------------------------------------ CubePad (bit-exact)
def test_cubepad_small_bit_exact(golden_dir):
    z = np.load(os.path.join(golden_dir, 'cubepad_small.npz'))
    for k in range(len(mg.CUBEPAD_SMALL)):
        x, y, pad = z['x%d' % k], z['y%d' % k], z['pad%d' % k]
        got = o_cubepad.cubepad(x, [int(v) for v in pad])
        assert got.shape == y.shape
        assert np.array_equal(got, y), 'case %d pad %s' % (k, pad)


def test_cubepad_hashed_bit_exact(golden_dir):
    want = json.load(open(os.path.join(golden_dir, 'cubepad_sha256.json')))
    for k, (n, p, C) in enumerate(mg.CUBEPAD_HASHED):
        x = mg.cubepad_input(n, C, 1, 2000 + k)
        assert sha(o_cubepad.cubepad(x, p)) == want['%d_%d_%d' % (n, p, C)]


def test_cubepad_reference_smoke_shape_and_hash(golden_dir):
    """The reference's only executable test (model/cube_pad.py:256-261): CubePad(2) on [12, 64, 256, 256] -> [12, 64, 260, 260]
    (seeded values instead of its zeros; hash of the reference's own output)."""
    want = json.load(open(os.path.join(golden_dir, 'cubepad_sha256.json')))
    n, p, C, groups = mg.CUBEPAD_SMOKE
    got = o_cubepad.cubepad(mg.cubepad_input(n, C, groups, 2100), p)
    assert got.shape == (12, 64, 260, 260)
    assert sha(got) == want['smoke_%d_%d_%d_x%d' % mg.CUBEPAD_SMOKE]


def test_cubepad_rejects_bad_batch():
    with pytest.raises(ValueError):
        o_cubepad.cubepad(np.zeros((5, 1, 4, 4), np.float32), 1)


# ------------------------------------------------------------------ Equi2Cube grids
@pytest.mark.parametrize('case', mg.E2C_CASES)
def test_e2c_grids_identical(golden_dir, case):
    H, W, cd = case
    meta = json.load(open(os.path.join(golden_dir, 'e2c_grids_sha256.json')))
    z = np.load(os.path.join(golden_dir, 'e2c_grids.npz'))
    key = '%dx%d_%d' % (H, W, cd)
    xs, ys = o_e2c.equi2cube_grids(cd, H, W)
    assert sha(np.stack([xs, ys])) == meta[key]['sha256_f64']      # float64 identical
    g = o_e2c.grids_f32(cd, H, W)
    assert sha(g) == meta[key]['sha256_f32']
    step = max(1, cd // 8)
    assert np.array_equal(g[:, ::step], z[key + '_rows'])


def test_remap_linear_known_answers():
    img = np.arange(20, dtype=np.float64).reshape(4, 5)
    mx = np.array([[0.0, 1.5, 3.999, 4.0, 2.015625]], dtype=np.float32)
    my = np.array([[0.0, 0.5, 1.0, 3.0, 2.984375]], dtype=np.float32)
    out = o_e2c.remap_linear(img, mx, my)
    # (0,0) exact; (1.5,0.5): mean of 1,2,6,7; x=3.999 rounds to 4.0 (1/32 grid): img[1,4];
    # (4,3): last pixel, the out-of-range taps carry weight 0; last: sx = 64.5 -> 64 and
    # sy = 95.5 -> 96 (round half to even) -> exactly img[3, 2]
    assert out[0, 0] == 0.0
    assert out[0, 1] == (1 + 2 + 6 + 7) / 4.0
    assert out[0, 2] == 9.0
    assert out[0, 3] == 19.0
    assert out[0, 4] == 17.0
    # plain-float mode interpolates instead of snapping to the 1/32 grid
    flt = o_e2c.remap_linear(img, mx, my, fixed_point=False)
    assert abs(flt[0, 2] - (8 + 0.999 * 1.0)) < 1e-5


# ------------------------------------------------------------------ Cube2Equi
@pytest.mark.parametrize('w', [4, 7, 8, 16])
def test_c2e_tables_and_sampling(golden_dir, w):
    z = np.load(os.path.join(golden_dir, 'c2e.npz'))
    face, coord = o_c2e.c2e_tables(w)
    assert np.array_equal(face.astype(np.int8), z['face_map_%d' % w])
    assert np.array_equal(coord, z['out_coord_%d' % w])
    assert o_c2e.grid_scale(coord) == z['M_%d' % w]
    got = o_c2e.to_equi_nn(z['nn_in_%d' % w], face, coord, align_corners=False)
    assert np.max(np.abs(got - z['nn_out_%d' % w])) <= 2e-6


def test_c2e_known_face_counts():
    # SURVEY.md 8(a10) anchors observed on the reference
    counts = {7: [36, 112, 36, 48, 48, 112], 8: [60, 136, 60, 60, 60, 136], 16: [236, 552, 236, 236, 236, 552]}
    for w, c in counts.items():
        face, _ = o_c2e.c2e_tables(w)
        assert [int((face == f).sum()) for f in range(6)] == c


# ------------------------------------------------------------------ ResNet-50-cubic + CAM
def _resnet_sd():
    return {k: torch.from_numpy(v) for k, v in synth.resnet50_state(seed=1).items()}


def test_resnet_cam_small(golden_dir):
    z = mg.load_resnet_cam(golden_dir)
    sd = _resnet_sd()
    cubes = mg.synth_cubes(4000 + 64, 64)
    chw = np.ascontiguousarray(np.transpose(cubes, (0, 3, 1, 2)))
    feat = o_resnet.resnet50_layer4(torch.from_numpy(chw), sd).numpy()
    assert feat.shape == (6, 2048, 2, 2)
    scale = np.abs(z['layer4_s']).max()
    assert np.max(np.abs(feat - z['layer4_s'])) <= 1e-5 * scale


@pytest.mark.slow
def test_resnet_cam_full(golden_dir):
    z = mg.load_resnet_cam(golden_dir)
    sd = _resnet_sd()
    cubes = mg.synth_cubes(4000 + 224, 224)
    chw = np.ascontiguousarray(np.transpose(cubes, (0, 3, 1, 2)))
    score, feat = o_resnet.cam_from_cubes(chw, sd)
    assert np.max(np.abs(feat[:, ::8] - z['layer4_f'])) <= 1e-5 * np.abs(z['layer4_f']).max()
    assert np.max(np.abs(score - z['cam_f'])) <= 1e-5 * np.abs(z['cam_f']).max()
    wsm = o_resnet.cam_weight(sd['fc.weight'].numpy())
    assert np.array_equal(wsm[::97, ::53], z['wsm_pick'])


# ------------------------------------------------------------------ ConvLSTM
def test_clstm_small_two_steps(golden_dir):
    z = np.load(os.path.join(golden_dir, 'clstm.npz'))
    sd = {k: torch.from_numpy(v) for k, v in synth.clstm_state(seed=7, input_size=8, hidden_size=8).items()}
    x = torch.from_numpy(hashrng.uniform(5000, (12, 8, 4, 4)))
    h = torch.from_numpy(hashrng.uniform(5001, (12, 8, 4, 4)))
    c = torch.from_numpy(hashrng.uniform(5002, (12, 8, 4, 4)))
    h1, c1 = o_clstm.clstm_step(x, h, c, sd)
    h2, c2 = o_clstm.clstm_step(x, h1, c1, sd)
    for got, key in ((h1, 'small_h1'), (c1, 'small_c1'), (h2, 'small_h2'), (c2, 'small_c2')):
        assert np.max(np.abs(got.numpy() - z[key])) <= 1e-6


@pytest.mark.slow
def test_clstm_full_window_T5(golden_dir):
    z = np.load(os.path.join(golden_dir, 'clstm.npz'))
    sd = {k: torch.from_numpy(v) for k, v in synth.clstm_state(seed=2).items()}
    frames = synth.cam_clip(6000 + 5, 5)
    hid = o_clstm.window_hidden(frames, sd)
    assert np.max(np.abs(hid.reshape(-1)[z['pick']] - z['full_hidden_pick_T5'])) <= 1e-4
    sal = o_c2e.saliency_from_hidden(hid)
    assert sal.shape == (14, 28)
    assert np.max(np.abs(sal - z['full_map_T5'])) <= 1e-4
