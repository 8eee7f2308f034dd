"""The launch paths of the resize, projection and glue kernels that no other GPU test takes (csrc/resize.hip,
csrc/misc.hip, csrc/projection.hip): each kernel against a plain CPU statement of the same operation, at the smallest
shapes that take the path.

Every comparison but one is bit-exact, for a reason that holds whatever the kernel's launch shape: the resize is integer
arithmetic; a maximum of representable values is representable; the window normalisation is one correctly rounded
subtraction and one correctly rounded division followed by round-to-nearest-even; a transpose moves values; the two paths
of the projection evaluate one expression on the same integer-valued taps.  The exception is the projection against
the float64 oracle, at the bound tests/test_gpu_parity.py::test_equi2cube_matches_oracle uses (2e-5)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from oracle import o_resize, o_resnet
from cp_360_weakly_supervised_saliency_amd import ops
from cp_360_weakly_supervised_saliency_amd.utils import hashrng, synth
from cp_360_weakly_supervised_saliency_amd.utils.equi_to_cube import Equi2Cube
from cp_360_weakly_supervised_saliency_amd.utils.resize import LanczosResize
from tests.golden import make_golden as mg
from tests import parity_helpers as ph
from tests.test_resize import side_path_frames

DEV = 'cuda'
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16


def bits(t):
    """The tensor's bytes, so that equality is bit for bit (NaN payloads and the sign of zero included)."""
    return t.contiguous().cpu().view(torch.uint8)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


# ------------------------------------------------------------------ K0 resize
def at_byte_offset(a, off, fill=0):
    """A contiguous device view of ``a`` (u8 numpy) whose storage starts ``off`` bytes into a fresh (aligned) allocation;
    also the whole buffer."""
    buf = torch.full((a.size + 8,), fill, dtype=torch.uint8, device=DEV)
    view = buf[off:off + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert buf.data_ptr() % 4 == 0 and view.data_ptr() % 4 == off % 4 and view.is_contiguous()
    return view, buf


def resize_case(in_hw, out_hw, plan, frames=None, filter='lanczos', in_off=0):
    """F = 2 differing frames through LanczosResize: the call takes the kernels of ``plan``, and each frame equals the
    oracle's resize of that frame."""
    frames = side_path_frames(in_hw) if frames is None else frames
    assert frames.shape[0] == 2 and not np.array_equal(frames[0], frames[1])
    r = LanczosResize(in_hw, out_hw, filter=filter)
    x, _ = at_byte_offset(frames, in_off)
    assert r.describe(x) == plan
    got = r(x).cpu().numpy()
    for f in range(2):
        assert np.array_equal(got[f], o_resize.resize_u8(frames[f], out_hw, filter)), (in_hw, out_hw, f)
    return got


def golden_case_frames(k):
    """Case k of the Pillow-made fixture and its vertical flip, as tests/test_resize.py::test_gpu_resize_bit_exact."""
    a = mg.resize_input(k)
    return np.stack([a, a[::-1].copy()])


@pytest.mark.gpu
def test_resize_bytewise_horizontal_pass_by_geometry():
    """A 4x horizontal shrink (25 taps): 256 outputs span 256 * 4 + 27 input pixels, more than the LDS kernel's 1024."""
    resize_case((9, 1000), (7, 250), 'horizontal bytewise, vertical bytewise')
    resize_case((9, 1000), (9, 250), 'horizontal bytewise, vertical none')        # straight into out, no intermediate


@pytest.mark.gpu
def test_resize_lds_window_horizontal_only_over_three_x_blocks():
    resize_case((5, 300), (5, 520), 'horizontal LDS window, vertical none')


@pytest.mark.gpu
@pytest.mark.parametrize('off', [1, 2])
def test_resize_misaligned_input_takes_the_bytewise_horizontal_pass(off, golden_dir):
    (in_hw, out_hw), frames = mg.RESIZE_CASES[3], golden_case_frames(3)
    got = resize_case(in_hw, out_hw, 'horizontal bytewise, vertical bytewise', frames=frames, in_off=off)
    assert np.array_equal(got[0], np.load(os.path.join(golden_dir, 'resize_lanczos.npz'))['y3'])      # Pillow's own


@pytest.mark.gpu
def test_resize_misaligned_out_takes_the_bytewise_vertical_pass(golden_dir):
    """Rows of 96 * 3 bytes (a multiple of 4) into an ``out`` one byte past an aligned address; the bytes around it stay."""
    (in_hw, out_hw), frames = mg.RESIZE_CASES[1], golden_case_frames(1)
    r = LanczosResize(in_hw, out_hw)
    x = torch.from_numpy(frames).to(DEV)
    assert r.describe(x) == 'horizontal none, vertical dword'
    out, buf = at_byte_offset(np.zeros((2,) + out_hw + (3,), np.uint8), 1, fill=0xA5)
    assert r.describe(x, out) == 'horizontal none, vertical bytewise'
    assert r(x, out=out) is out
    whole = buf.cpu().numpy()
    got = whole[1:1 + out.numel()].reshape(out.shape)
    for f in range(2):
        assert np.array_equal(got[f], o_resize.resize_lanczos_u8(frames[f], out_hw)), f
    assert np.array_equal(got[0], np.load(os.path.join(golden_dir, 'resize_lanczos.npz'))['y1'])
    assert np.all(whole[:1] == 0xA5) and np.all(whole[1 + out.numel():] == 0xA5)
    assert np.array_equal(r(x).cpu().numpy(), got)                    # the dword pass on the same frames


@pytest.mark.gpu
def test_resize_identity_is_a_copy_into_the_callers_out():
    frames = side_path_frames((12, 20))
    r = LanczosResize((12, 20), (12, 20))
    x = torch.from_numpy(frames).to(DEV)
    out = torch.full((2, 12, 20, 3), 0xA5, dtype=torch.uint8, device=DEV)
    assert r.describe(x, out) == 'copy'
    assert r(x, out=out) is out and np.array_equal(out.cpu().numpy(), frames)
    assert out.data_ptr() != x.data_ptr() and np.array_equal(x.cpu().numpy(), frames)


@pytest.mark.gpu
def test_resize_bicubic_upsample():
    resize_case((14, 28), (96, 192), 'horizontal LDS window, vertical dword', filter='bicubic')


# ------------------------------------------------------------------ K7 window min / max
def minmax(x, B, per_clip, clip_stride=0):
    mm = torch.empty((B, 2), device=DEV)
    scratch = torch.empty((B * 512,), device=DEV)
    ops.window_minmax(x, B, per_clip, mm, scratch, clip_stride)
    return mm.cpu().numpy()


@pytest.mark.gpu
def test_window_minmax_poisoned_by_one_non_finite_value():
    """The contract in csrc/misc.hip: a window that holds an inf or a NaN gets min = max = NaN (fminf / fmaxf alone would
    drop a NaN and keep an inf), wherever the value sits - every lane of a float4, the last vector, a vector of the
    first pass's second sweep (70000 vectors for 256 x 256 threads) - and the neighbouring windows stay exact."""
    B, per_clip = 3, 4 * 70000
    x = hashrng.normal(8301, (B, per_clip), 5.0, 100.0)
    xt = torch.from_numpy(x).to(DEV)
    lo, hi = x.min(1), x.max(1)
    got = minmax(xt, B, per_clip)
    assert np.array_equal(got[:, 0], lo) and np.array_equal(got[:, 1], hi)
    middle = 4 * (256 * 37 + 5) + 2                                   # lane z of a vector that workgroup 37 owns
    for pos in (0, 1, 2, 3, per_clip - 1, middle):
        for bad in (np.inf, -np.inf, np.nan):
            keep = float(x[1, pos])
            xt[1, pos] = bad
            got = minmax(xt, B, per_clip)
            xt[1, pos] = keep
            assert np.isnan(got[1, 0]) and np.isnan(got[1, 1]), (pos, bad, got[1])
            assert np.array_equal(got[[0, 2], 0], lo[[0, 2]]) and np.array_equal(got[[0, 2], 1], hi[[0, 2]]), (pos, bad)
    got = minmax(xt, B, per_clip)                                     # restored: finite again
    assert np.array_equal(got[:, 0], lo) and np.array_equal(got[:, 1], hi)


@pytest.mark.gpu
def test_window_minmax_sliding_windows_single_vector_and_alignment():
    B, T, P, C = 4, 3, 294, 8
    seq = hashrng.normal(8302, ((B + T - 1) * P * C,), -3.0, 50.0)    # one sequence; window b = frames b .. b + T - 1
    st = torch.from_numpy(seq).to(DEV)
    got = minmax(st, B, T * P * C, clip_stride=P * C)
    for b in range(B):
        w = seq[b * P * C: b * P * C + T * P * C]
        assert got[b, 0] == w.min() and got[b, 1] == w.max(), b
    got = minmax(st, 3, 4, clip_stride=8)                             # per_clip = 4: one vector per window
    for b in range(3):
        assert got[b, 0] == seq[8 * b: 8 * b + 4].min() and got[b, 1] == seq[8 * b: 8 * b + 4].max(), b
    got = minmax(st, 5, 4)                                            # clip_stride 0 = dense
    assert np.array_equal(got[:, 0], seq[:20].reshape(5, 4).min(1)) and np.array_equal(got[:, 1], seq[:20].reshape(5, 4).max(1))
    with pytest.raises(ValueError, match='status -6'):                # CP360_ERR_ALIGN
        minmax(st, 2, 6, clip_stride=8)
    with pytest.raises(ValueError, match='status -6'):
        minmax(st, 2, 8, clip_stride=6)


# ------------------------------------------------------------------ K7 window normalise
def normalised(x, mn, mx):
    """(x - mn) / (mx - mn) in float32: one rounded subtraction, one rounded division (numpy's float32 arithmetic)."""
    mn, mx = np.float32(mn), np.float32(mx)
    want = (x - mn) / (mx - mn)
    assert want.dtype == np.float32
    return torch.from_numpy(want)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [F32, BF16, F16])
def test_window_normalize_every_output_type_bit_exact(dtype):
    B, T, P, C, t = 2, 3, 37, 20, 1
    x = hashrng.normal(8303, (B, T, P, C), 5.0, 100.0)
    xt = torch.from_numpy(x).to(DEV)
    mm_np = np.stack([x.reshape(B, -1).min(1), x.reshape(B, -1).max(1)], 1)
    mm = torch.from_numpy(mm_np).to(DEV)
    want = torch.stack([normalised(x[b, t], *mm_np[b]) for b in range(B)])              # f32 [B, P, C]
    for coff in (0, C):
        for with_y2 in (True, False):
            y = torch.zeros((B, P, 2 * C), dtype=dtype, device=DEV)
            y2 = torch.full((B, P, C), -7.0, device=DEV) if with_y2 else None
            ops.window_normalize(xt, mm, y, coff, y2, B, T, t, P, C)
            assert same_bits(y[:, :, coff:coff + C], want.to(dtype)), (coff, with_y2)
            assert not y[:, :, C - coff:2 * C - coff].any()                                # the other half: untouched
            if with_y2:
                assert same_bits(y2, want)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [F32, BF16, F16])
def test_window_normalize_frames_bit_exact(dtype):
    """cp360_window_normalize_frames: one grid layer per frame, 294 * 250 vectors for at most 256 x 256 threads (the
    grid-stride loop iterates); dense windows and windows sliding over one sequence."""
    B, T, P, C = 2, 3, 294, 1000
    seq = normalize_frames_input()
    for stride in (0, P * C):
        step = stride or T * P * C
        wins = [seq[b * step: b * step + T * P * C].reshape(T, P, C) for b in range(B)]
        mm_np = np.array([[w.min(), w.max()] for w in wins], np.float32)
        want = torch.stack([normalised(w, *m) for w, m in zip(wins, mm_np)], 1)        # [T, B, P, C]
        y = torch.zeros((T, B, P, C), dtype=dtype, device=DEV)
        ops.window_normalize_frames(torch.from_numpy(seq).to(DEV), torch.from_numpy(mm_np).to(DEV), y, B, T, P, C, stride)
        assert same_bits(y, want.to(dtype)), stride


_NF_INPUT = []


def normalize_frames_input():
    if not _NF_INPUT:
        _NF_INPUT.append(hashrng.normal(8304, (2 * 3 * 294 * 1000,), 5.0, 100.0))
    return _NF_INPUT[0]


# ------------------------------------------------------------------ K3b CubePad + max-pool
def maxpool_reference(x):
    """x [6N, n, n, C] CPU, already rounded to its type -> CubePad(1) + MaxPool2d(3, 2, 0), NHWC, same type (a maximum of
    representable values: exact)."""
    y = Fn.max_pool2d(o_resnet.cubepad_t(x.float().permute(0, 3, 1, 2).contiguous(), 1), 3, 2, 0)
    return y.permute(0, 2, 3, 1).contiguous().to(x.dtype)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype,C', [(F32, 4), (F32, 20), (BF16, 8), (F16, 8), (BF16, 12), (F16, 12), (BF16, 64)])
def test_cubepad_maxpool_against_the_oracle(dtype, C):
    """Even and odd faces (the last window of an odd face reads the pad), n = 2, one and two cubes; all-negative inputs,
    so a tap missed at a face border shows against the -inf start value; the 16-byte kernel in both launch orders."""
    for n in (2, 3, 7, 8, 9, 14):
        for n6 in (6, 12):
            x = torch.from_numpy(hashrng.normal(8400 + n * 13 + n6, (n6, n, n, C)) - 6.0).to(dtype)
            assert bool((x < 0).all())
            want = maxpool_reference(x)
            assert want.shape == (n6, (n - 1) // 2 + 1, (n - 1) // 2 + 1, C)
            xd = x.to(DEV)
            for order in ((0, 1) if dtype != F32 and C % 8 == 0 else (0,)):
                with ops.launch_order(order):
                    got = ops.cubepad_maxpool3s2(xd)
                assert same_bits(got, want), (n, n6, order)


@pytest.mark.gpu
def test_cubepad_maxpool_refusals():
    with pytest.raises(ValueError, match='status -2'):                # CP360_ERR_BATCH_NOT_6N
        ops.cubepad_maxpool3s2(torch.zeros((5, 4, 4, 8), device=DEV))
    with pytest.raises(ValueError, match='status -6'):                # CP360_ERR_ALIGN
        ops.cubepad_maxpool3s2(torch.zeros((6, 4, 4, 6), device=DEV))


# ------------------------------------------------------------------ layout transposes
TRANSPOSE_PAIRS = [(F32, F32), (F32, BF16), (F32, F16), (BF16, F32), (BF16, BF16), (F16, F32), (F16, F16)]
# tiles below 32, exactly 32, one past 32, a single row
TRANSPOSE_SHAPES = [(1, 3, 2, 2), (2, 32, 4, 8), (3, 33, 5, 13), (2, 70, 1, 31)]


@pytest.mark.gpu
@pytest.mark.parametrize('din,dout', TRANSPOSE_PAIRS, ids=lambda d: str(d).replace('torch.', ''))
def test_transposes_every_dtype_pair_both_directions(din, dout):
    for k, (N, C, H, W) in enumerate(TRANSPOSE_SHAPES):
        x = torch.from_numpy(hashrng.normal(8500 + k, (N, C, H, W), 0.0, 30.0)).to(din)          # NCHW, as the kernel reads it
        x_nhwc = x.permute(0, 2, 3, 1).contiguous()
        # NCHW -> NHWC: dense, and into channels [4, 4 + C) of a wider pixel
        assert same_bits(ops.nchw_to_nhwc(x.to(DEV), out_dtype=dout), x_nhwc.to(dout)), (k, 'to nhwc')
        ld, coff = C + 11, 4
        wide = torch.full((N, H, W, ld), 7.0, dtype=dout, device=DEV)
        ops.nchw_to_nhwc(x.to(DEV), out=wide, coff=coff)
        assert same_bits(wide[..., coff:coff + C], x_nhwc.to(dout)), (k, 'to nhwc slice')
        assert bool((wide[..., :coff] == 7.0).all()) and bool((wide[..., coff + C:] == 7.0).all()), k
        # NHWC -> NCHW: dense, and from that channel slice (the sentinel around it must not come through)
        assert same_bits(ops.nhwc_to_nchw(x_nhwc.to(DEV), out_dtype=dout), x.to(dout)), (k, 'to nchw')
        src = torch.full((N, H, W, ld), 999.0, dtype=din)
        src[..., coff:coff + C] = x_nhwc
        assert same_bits(ops.nhwc_to_nchw(src.to(DEV), out_dtype=dout, channels=C, coff=coff), x.to(dout)), (k, 'to nchw slice')


@pytest.mark.gpu
def test_transpose_refusals():
    x = torch.zeros((2, 8, 3, 3), device=DEV)
    with pytest.raises(ValueError, match='status -1'):                # ld < C + coff: CP360_ERR_BAD_SHAPE
        ops.nchw_to_nhwc(x, out=torch.zeros((2, 3, 3, 10), device=DEV), coff=4)
    with pytest.raises(ValueError, match='status -1'):
        ops.nhwc_to_nchw(torch.zeros((2, 3, 3, 10), device=DEV), channels=8, coff=4)
    with pytest.raises(ValueError, match='status -4'):                # bf16 -> fp16 is not dispatched: CP360_ERR_BAD_DTYPE
        ops.nchw_to_nhwc(x.to(BF16), out_dtype=F16)
    with pytest.raises(ValueError, match='status -4'):
        ops.nhwc_to_nchw(x.to(BF16), out_dtype=F16)


# ------------------------------------------------------------------ K1 equi -> cube
def e2c_frames(F, H, W):
    return np.stack([synth.frame_u8(8600 + i, H, W) for i in range(F)])


@pytest.mark.gpu
@pytest.mark.parametrize('H,W,cd', [(63, 126, 16), (8, 16, 4)])
def test_equi2cube_u8_fast_path_equals_the_guarded_path(H, W, cd):
    """u8 frames (12-byte aligned loads + funnel shift wherever ix + 4 < W) against the same frames as floats (every tap
    through the guarded loads), bit for bit: the taps are the same integers and the expression is the same.  H = 63: the
    frame stride H * W * 3 is 2 mod 4, so every frame starts at another byte phase; F = 6: two frame groups, the second
    with two live frames.  8 x 16: ix + 4 < W fails for three pixels in eight, which take the guarded path in u8 too."""
    F = 6
    assert (H * W * 3) % 4 == (2 if H == 63 else 0)
    frames = e2c_frames(F, H, W)
    e = Equi2Cube(cd, (H, W))
    ft = torch.from_numpy(frames).to(DEV)
    for layout in ('nchw', 'nhwc4'):
        got = ops.equi2cube(ft, e.grid, cd, F32, layout)
        slow = ops.equi2cube(ft.float(), e.grid, cd, F32, layout, scale=1.0 / 255.0)
        assert same_bits(got, slow), layout
    got = ops.equi2cube(ft, e.grid, cd, F32, 'nchw').cpu().numpy().reshape(F, 6, 3, cd, cd)
    for f in range(F):
        assert np.max(np.abs(got[f] - ph.oracle_cubes(frames[f], cd))) <= 2e-5, f


@pytest.mark.gpu
def test_equi2cube_scale_with_16_bit_outputs():
    """Float frames in [0, 255] with scale = 1 / 255: the bf16 / fp16 outputs are the f32 output rounded once."""
    H, W, cd, F = 64, 128, 16, 2
    e = Equi2Cube(cd, (H, W))
    ft = torch.from_numpy(e2c_frames(F, H, W)).to(DEV).float()
    for layout in ('nchw', 'nhwc4'):
        ref = ops.equi2cube(ft, e.grid, cd, F32, layout, scale=1.0 / 255.0).cpu()
        unscaled = ops.equi2cube(ft, e.grid, cd, F32, layout).cpu()
        assert not torch.equal(ref, unscaled)                         # the argument is used
        for dt in (BF16, F16):
            got = ops.equi2cube(ft, e.grid, cd, dt, layout, scale=1.0 / 255.0)
            assert same_bits(got, ref.to(dt)), (layout, dt)
            if layout == 'nhwc4':
                assert not got[..., 3].any()


@pytest.mark.gpu
@pytest.mark.parametrize('F', [4, 5, 7, 8])
def test_equi2cube_ragged_frame_groups(F):
    """Frame k of a batch (threads own groups of 4 frames; the last group may be ragged) == that frame run alone."""
    H, W, cd = 64, 128, 16
    e = Equi2Cube(cd, (H, W))
    ft = torch.from_numpy(e2c_frames(8, H, W)[:F]).to(DEV)
    for layout in ('nchw', 'nhwc4'):
        got = ops.equi2cube(ft, e.grid, cd, F32, layout)
        assert got.shape[0] == 6 * F
        for k in range(F):
            assert same_bits(got[6 * k:6 * k + 6], ops.equi2cube(ft[k:k + 1], e.grid, cd, F32, layout)), (layout, k)


# ------------------------------------------------------------------ the fused kernels' weight packers
# Each packer against a numpy restatement of the layout comment above its kernel (csrc/l1block.hip, l2block.hip, lfirst.hip,
# band3x3.hip, stem.hip), bit for bit.  Scales are None or signed powers of two, so the f32 product with the BN scale is exact
# and the expected bytes do not depend on whether a packer rounds that product before the 16-bit conversion.
def row_chan(R):
    """Packed row R of a 32-row group holds this channel (csrc/tile.h): row 32q + 16b + 4g + e <- channel 32q + 8g + 4b + e."""
    return (R & ~31) + ((R >> 2) & 3) * 8 + ((R >> 4) & 1) * 4 + (R & 3)


def frag_lane(idx):
    """idx -> (fragment, row inside its 16-row block, first channel of the lane's k-group + e): a fragment is [lane 64][e 8],
    lane l holds row l & 15, k-group l >> 4."""
    e, lane = idx & 7, (idx >> 3) & 63
    return idx >> 9, lane & 15, (lane >> 4) * 8 + e


def want_frag_1x1(w, n_out, k, order):
    frag, row, kc = frag_lane(np.arange(n_out * k))
    KB, RB = k // 32, n_out // 16
    rb, kb = (frag // KB, frag % KB) if order == 0 else (frag % RB, frag // RB)
    return w[row_chan(rb * 16 + row), kb * 32 + kc]


def want_l1_conv2(w):                                   # [tap 9][row block 4][kk 2][lane][8]
    frag, row, kc = frag_lane(np.arange(9 * 64 * 64))
    kk, rb, tap = frag & 1, (frag >> 1) & 3, frag >> 3
    return w.reshape(64, 64, 9)[row_chan(rb * 16 + row), kk * 32 + kc, tap]


def want_bt_conv2(w, c):                                # [channel half][step = tap * SPT + sub][wave 4][i 2][kk 2][lane][8]
    spt = c // 64
    frag, row, kc = frag_lane(np.arange(9 * c * c))
    kk, i, wv, rest = frag & 1, (frag >> 1) & 1, (frag >> 2) & 3, frag >> 4
    st, hc = rest % (9 * spt), rest // (9 * spt)
    tap, sub = st // spt, st % spt
    return w.reshape(c, c, 9)[row_chan(((hc * 4 + wv) * 2 + i) * 16 + row), (sub * 2 + kk) * 32 + kc, tap]


def want_w3d(w3d):                                      # [W3 | Wd] [512, 384]: fragment (p * 2 + rb) * 12 + kb, 32-row pair p
    frag, row, kc = frag_lane(np.arange(512 * 384))     # (written out from its own comment, not through want_frag_1x1)
    kb, rb, p = frag % 12, (frag // 12) & 1, frag // 24
    return w3d[row_chan(p * 32 + rb * 16 + row), kb * 32 + kc]


def want_band3x3(w):                                    # [tap][row r][64 channels]
    idx = np.arange(9 * 64 * 64)
    return w.reshape(64, 64, 9)[row_chan((idx >> 6) & 63), idx & 63, idx >> 12]


def want_stem(w):                                       # [ky][row r][k = kx * 4 + ch], kx < 7 and ch < 3, the rest zero
    idx = np.arange(7 * 64 * 32)
    k, r, ky = idx & 31, (idx >> 5) & 63, idx >> 11
    kx, ch = k >> 2, k & 3
    ok = (kx < 7) & (ch < 3)
    return np.where(ok, w[row_chan(r), np.minimum(ch, 2), ky, np.minimum(kx, 6)], np.float32(0))


def pow2_scale(seed, n):
    """n signed powers of two in [2^-3, 2^3]."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 2, (n,), generator=g) * 2 - 1).float() * torch.exp2(torch.randint(-3, 4, (n,), generator=g).float())


def packer_cases():
    """(name, weight shapes, channels the scale runs over, call(L, code, weights, scales, out) -> status, restatement)."""
    from cp_360_weakly_supervised_saliency_amd._lib import ptr, stream
    cases = []
    for n_out, k in ((32, 32), (64, 256)):
        for order in (0, 1):
            cases.append(('frag_%dx%d_o%d' % (n_out, k, order), [(n_out, k)],
                          lambda L, c, w, s, o, n_out=n_out, k=k, order=order:
                          L.cp360_frag_pack_1x1(c, ptr(w[0]), ptr(s[0]), ptr(o), n_out, k, order, stream()),
                          lambda w, n_out=n_out, k=k, order=order: want_frag_1x1(w[0], n_out, k, order)))
    simple = (('l1_conv2', (64, 64, 3, 3), 'cp360_l1block_pack_conv2', want_l1_conv2),
              ('l2_conv2', (128, 128, 3, 3), 'cp360_l2block_pack_weights', lambda w: want_bt_conv2(w, 128)),
              ('l3_conv2', (256, 256, 3, 3), 'cp360_l3block_pack_weights', lambda w: want_bt_conv2(w, 256)),
              ('band3x3', (64, 64, 3, 3), 'cp360_band3x3_pack_weights', want_band3x3),
              ('stem', (64, 3, 7, 7), 'cp360_stem_pack_weights', want_stem))
    for name, shape, fn, want in simple:
        cases.append((name, [shape], lambda L, c, w, s, o, fn=fn: getattr(L, fn)(c, ptr(w[0]), ptr(s[0]), ptr(o), stream()),
                      lambda w, want=want: want(w[0])))
    cases.append(('l2first_w3d', [(512, 128), (512, 256)],
                  lambda L, c, w, s, o: L.cp360_l2first_pack_w3d(c, ptr(w[0]), ptr(s[0]), ptr(w[1]), ptr(s[1]), ptr(o), stream()),
                  lambda w: want_w3d(np.concatenate([w[0], w[1]], axis=1))))
    return cases


@pytest.mark.gpu
def test_fused_packers_layouts_bit_exact():
    from cp_360_weakly_supervised_saliency_amd import _lib
    L = _lib.lib()
    BAD_DTYPE = -4                                      # CP360_ERR_BAD_DTYPE (include/cp360.h)
    assert L.cp360_frag_packed_bytes(_lib.BF16, 48, 32) == 0 and L.cp360_frag_packed_bytes(_lib.F32, 32, 32) == 0
    for ci, (name, shapes, call, want) in enumerate(packer_cases()):
        g = torch.Generator().manual_seed(100 + ci)
        ws = [torch.randn(s, generator=g) for s in shapes]
        for scaled in (False, True):
            scs = [pow2_scale(200 + ci + 50 * i, s[0]) if scaled else None for i, s in enumerate(shapes)]
            # the folded weights in f32 (exact: the scales are powers of two), then the restated layout
            folded = [(w if sc is None else w * sc.reshape(-1, *([1] * (w.dim() - 1)))).numpy() for w, sc in zip(ws, scs)]
            flat = torch.from_numpy(np.ascontiguousarray(want(folded), dtype=np.float32))
            dw = [w.to(DEV) for w in ws]
            dsc = [None if sc is None else sc.to(DEV) for sc in scs]
            for dt, code in ((BF16, _lib.BF16), (F16, _lib.F16)):
                out = torch.full((flat.numel() * 2,), 0xA5, dtype=torch.uint8, device=DEV)
                assert call(L, code, dw, dsc, out) == 0, (name, dt)
                torch.cuda.synchronize()
                assert torch.equal(out.cpu(), bits(flat.to(dt)).reshape(-1)), (name, dt, scaled)
            out = torch.zeros(flat.numel() * 2, dtype=torch.uint8, device=DEV)
            assert call(L, _lib.F32, dw, dsc, out) == BAD_DTYPE, name
