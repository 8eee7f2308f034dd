"""Frame resize: dataset_feat_extractor.py:131-133 resizes every frame with PIL's
LANCZOS filter.  The oracle restatement is pinned against Pillow itself (golden fixture made with the real
library + a live comparison when Pillow is importable); the HIP kernels are bit-exact against both."""
import os

import numpy as np
import pytest
import torch

from oracle import o_resize
from cp_360_weakly_supervised_saliency_amd.utils import hashrng
from cp_360_weakly_supervised_saliency_amd.utils.resize import LanczosResize, lanczos_tables
from tests.golden import make_golden as mg


def test_oracle_resize_matches_pillow_golden(golden_dir):
    z = np.load(os.path.join(golden_dir, 'resize_lanczos.npz'))
    for k, (_, out_hw) in enumerate(mg.RESIZE_CASES):
        got = o_resize.resize_lanczos_u8(mg.resize_input(k), out_hw)
        assert got.dtype == np.uint8 and np.array_equal(got, z['y%d' % k]), k


def test_oracle_resize_matches_live_pillow():
    Image = pytest.importorskip('PIL.Image')
    for k, ((h, w), (oh, ow)) in enumerate([((120, 250), (64, 128)), ((33, 77), (99, 50)), ((40, 40), (40, 17))]):
        a = hashrng.uniform(7100 + k, (h, w, 3), 0.0, 256.0).astype(np.uint8)
        want = np.array(Image.fromarray(a).convert('RGB').resize((ow, oh), resample=Image.LANCZOS))
        assert np.array_equal(o_resize.resize_lanczos_u8(a, (oh, ow)), want)


@pytest.mark.parametrize('sizes', [(750, 512), (376, 256), (200, 256), (2160, 960), (3840, 1920), (7, 3), (5, 5)])
def test_host_tables_equal_oracle(sizes):
    """cp360_resize_coeffs_host (C, libm) == the oracle's tables (python floats), integer for integer."""
    bo, ko = o_resize.precompute_coeffs(*sizes)
    bl, kl = lanczos_tables(*sizes)
    assert np.array_equal(bo, bl) and np.array_equal(ko, kl)
    assert np.all(ko.sum(1) >= (1 << 22) - 8) and np.all(ko.sum(1) <= (1 << 22) + 8)     # weights sum to 1


# The geometries of tests/test_side_paths_gpu.py (each takes another pair of kernels) and the full-size frame resize:
# ((h_in, w_in), (h_out, w_out), filter, byte offset of the input, byte offset of the output, the pair expected)
RESIZE_PLANS = [
    ((9, 1000), (7, 250), 'lanczos', 0, 0, 'horizontal bytewise, vertical bytewise'),      # 256 * 4 + 25 + 2 > 1024 pixels
    ((9, 1000), (9, 250), 'lanczos', 0, 0, 'horizontal bytewise, vertical none'),
    ((5, 300), (5, 520), 'lanczos', 0, 0, 'horizontal LDS window, vertical none'),
    ((97, 131), (61, 203), 'lanczos', 0, 0, 'horizontal LDS window, vertical bytewise'),   # 203 * 3 % 4 != 0
    ((97, 131), (61, 203), 'lanczos', 1, 0, 'horizontal bytewise, vertical bytewise'),
    ((97, 131), (61, 203), 'lanczos', 2, 0, 'horizontal bytewise, vertical bytewise'),
    ((54, 96), (48, 96), 'lanczos', 0, 0, 'horizontal none, vertical dword'),
    ((54, 96), (48, 96), 'lanczos', 0, 1, 'horizontal none, vertical bytewise'),
    ((54, 96), (48, 96), 'lanczos', 2, 0, 'horizontal none, vertical bytewise'),           # the vertical pass reads the input
    ((12, 20), (12, 20), 'lanczos', 0, 0, 'copy'),
    ((12, 20), (12, 20), 'lanczos', 1, 3, 'copy'),
    ((14, 28), (96, 192), 'bicubic', 0, 0, 'horizontal LDS window, vertical dword'),
    ((1080, 2160), (960, 1920), 'lanczos', 0, 0, 'horizontal LDS window, vertical dword'),
]


def _resize_plan(in_hw, out_hw, filter='lanczos', in_off=0, out_off=0, tmp_off=0, F=2):
    """cp360_resize_plan_describe on made-up addresses (it reads their alignment only): no GPU."""
    import ctypes as C
    from cp_360_weakly_supervised_saliency_amd._lib import check, lib
    from cp_360_weakly_supervised_saliency_amd.utils.resize import FILTERS
    L = lib()
    hks = L.cp360_resize_ksize2(in_hw[1], out_hw[1], FILTERS[filter]) if in_hw[1] != out_hw[1] else 0
    vks = L.cp360_resize_ksize2(in_hw[0], out_hw[0], FILTERS[filter]) if in_hw[0] != out_hw[0] else 0
    buf = C.create_string_buffer(96)
    n = L.cp360_resize_plan_describe(C.c_void_p(4096 + in_off), C.c_void_p(8192 + out_off), C.c_void_p(12288 + tmp_off), F,
                                     in_hw[0], in_hw[1], out_hw[0], out_hw[1], hks, vks, buf, len(buf))
    if n < 0:
        check(n)
    assert n == len(buf.value)
    return buf.value.decode()


def test_resize_plan_names_the_kernels_of_every_geometry():
    """cp360_resize_plan_describe (the record cp360_resize_lanczos_u8 launches from) for the geometries the GPU tests run and
    the full-size frame resize: today's choice of kernels, pinned."""
    for in_hw, out_hw, filt, in_off, out_off, want in RESIZE_PLANS:
        assert _resize_plan(in_hw, out_hw, filt, in_off, out_off) == want, (in_hw, out_hw, filt, in_off, out_off)
    # a misaligned intermediate of a two-pass resize, and F * h_in rows past the LDS kernel's 2^24 row items
    assert _resize_plan((54, 100), (48, 96), tmp_off=1) == 'horizontal LDS window, vertical bytewise'
    assert _resize_plan((54, 100), (48, 96)) == 'horizontal LDS window, vertical dword'
    assert _resize_plan((8, 100), (8, 96), F=1 << 21) == 'horizontal bytewise, vertical none'
    assert _resize_plan((8, 100), (8, 96), F=(1 << 21) - 1) == 'horizontal LDS window, vertical none'
    # refusals come back as the call's own status codes, and a short buffer truncates
    import ctypes as C
    from cp_360_weakly_supervised_saliency_amd._lib import lib
    L, one, buf = lib(), C.c_void_p(16), C.create_string_buffer(96)
    assert L.cp360_resize_plan_describe(None, one, None, 1, 4, 4, 2, 2, 7, 7, buf, 96) == -5
    assert L.cp360_resize_plan_describe(one, one, None, 1, 4, 4, 2, 2, 7, 7, buf, 96) == -5          # both axes: tmp
    assert L.cp360_resize_plan_describe(one, one, one, 0, 4, 4, 2, 2, 7, 7, buf, 96) == -1
    assert L.cp360_resize_plan_describe(one, one, one, 1, 4, 4, 2, 2, 7, 7, None, 0) == -5
    assert L.cp360_resize_plan_describe(one, one, one, 1, 4, 4, 4, 4, 0, 0, buf, 3) == 2 and buf.value == b'co'


def test_oracle_resize_matches_live_pillow_on_the_side_path_geometries():
    """The oracle against Pillow itself at the geometries of tests/test_side_paths_gpu.py (a 4x horizontal shrink with 25
    taps, horizontal-only resizes, the bicubic upsample), on the inputs those tests use."""
    Image = pytest.importorskip('PIL.Image')
    for in_hw, out_hw, filt, _, _, _ in RESIZE_PLANS[:-1]:
        a = side_path_frames(in_hw)[1]
        resample = Image.LANCZOS if filt == 'lanczos' else Image.BICUBIC
        want = np.array(Image.fromarray(a).convert('RGB').resize((out_hw[1], out_hw[0]), resample=resample))
        assert np.array_equal(o_resize.resize_u8(a, out_hw, filt), want), (in_hw, out_hw, filt)


def side_path_frames(in_hw, F=2):
    """The seeded u8 frames [F, h, w, 3] of a side-path resize case (the frames differ)."""
    return hashrng.uniform(7300 + in_hw[0] * 7 + in_hw[1], (F,) + tuple(in_hw) + (3,), 0.0, 256.0).astype(np.uint8)


@pytest.mark.gpu
def test_gpu_resize_bit_exact(golden_dir):
    z = np.load(os.path.join(golden_dir, 'resize_lanczos.npz'))
    for k, ((h, w), out_hw) in enumerate(mg.RESIZE_CASES):
        a = mg.resize_input(k)
        frames = torch.from_numpy(np.stack([a, a[::-1].copy()])).cuda()          # F = 2
        got = LanczosResize((h, w), out_hw)(frames).cpu().numpy()
        assert np.array_equal(got[0], z['y%d' % k]), k
        assert np.array_equal(got[1], o_resize.resize_lanczos_u8(a[::-1].copy(), out_hw)), k


@pytest.mark.gpu
def test_gpu_resize_full_size_against_pillow_or_oracle():
    """1080x2160 -> 960x1920 (the reference's cfg.equi_w x cfg.equi_h target), one frame."""
    a = hashrng.uniform(7200, (1080, 2160, 3), 0.0, 256.0).astype(np.uint8)
    got = LanczosResize((1080, 2160), (960, 1920))(torch.from_numpy(a[None]).cuda()).cpu().numpy()[0]
    try:
        from PIL import Image
        want = np.array(Image.fromarray(a).convert('RGB').resize((1920, 960), resample=Image.LANCZOS))
    except ImportError:
        want = o_resize.resize_lanczos_u8(a, (960, 1920))
    assert np.array_equal(got, want)
    with pytest.raises(ValueError):
        LanczosResize((1080, 2160), (960, 1920))(torch.zeros((1, 10, 10, 3), dtype=torch.uint8).cuda())


@pytest.mark.gpu
def test_pipeline_with_source_resize_matches_oracle():
    """Decoded 300x600 frames -> K0 resize to 256x512 -> the rest of the path, against the oracle fed with
    the oracle-resized frames (fp32, 1e-3 on the saliency map)."""
    from cp_360_weakly_supervised_saliency_amd.pipeline import SaliencyEngine
    from cp_360_weakly_supervised_saliency_amd.utils import synth
    from tests.parity_helpers import oracle_pipeline
    Hs, Ws, H, W, cd, T = 300, 600, 256, 512, 64, 2
    rs, cs = synth.resnet50_state(seed=1), synth.clstm_state(seed=3)
    clip = synth.clip_u8(60, T, Hs, Ws)
    small = np.stack([o_resize.resize_lanczos_u8(f, (H, W)) for f in clip])
    ref = oracle_pipeline(small, rs, cs, cd)
    eng = SaliencyEngine(rs, cs, (H, W), cd, clips=1, frames=T, precision='fp32', source_hw=(Hs, Ws))
    sal = eng(torch.from_numpy(clip[None]).cuda()).cpu().numpy()[0]
    assert np.max(np.abs(sal - ref)) <= 1e-3
