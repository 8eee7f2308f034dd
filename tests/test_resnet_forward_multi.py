"""cp360_resnet_forward_multi (csrc/ctx.hip): the static stages of several in-flight batches with the 14x14 and 7x7 layers
(layer3.1 .. layer4, the CAM) as ONE pass, and SaliencyEngine.stream() on top of it.

The back half runs the launches of the plan at one batch's face count with the image count replaced: the same kernel family,
split-K count, K ranges, finish order and epilogue; GEMM rows are independent and CubePad stays inside a cube.  So every
batch's CAM must be cp360_resnet_forward's bit for bit - the tests ask for equality, not a tolerance.  Cube 224 throughout (the
fused 14x14 tail kernels run), 128 x 256 equirectangular frames.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from cp_360_weakly_supervised_saliency_amd import _lib, stage_ctx
from cp_360_weakly_supervised_saliency_amd.model.resnet_cubic import resnet50
from cp_360_weakly_supervised_saliency_amd.utils import synth
from cp_360_weakly_supervised_saliency_amd.utils.equi_to_cube import Equi2Cube

pytestmark = pytest.mark.gpu
H, W, CD, HW, NC = 128, 256, 224, 7, 1000


@pytest.fixture(scope='module')
def resnet_state():
    return synth.resnet50_state(seed=1)


class _Net:
    """One loaded static stage of a 16-bit type, faces of 8 distinct frames, and the plain forward of every face set used."""

    def __init__(self, state, prec):
        self.dt = _lib.precision_dtype(prec)
        self.model = resnet50(precision=prec)
        self.model.load_state_dict({k: v if torch.is_tensor(v) else torch.from_numpy(v) for k, v in state.items()}, strict=False)
        self.model.cuda().eval()
        self.stage = stage_ctx.ResnetStage(self.model)
        self.stage._load()
        self.h = self.stage.ctx.h
        e2c = Equi2Cube(CD, (H, W), device='cuda')
        frames = torch.from_numpy(synth.clip_u8(70, 8, H, W)).cuda()
        with torch.no_grad():
            self.faces = e2c.to_cube_batch(frames, out_dtype=self.dt, layout='nhwc4p3')      # [48, 230, 230, 4]
        self._plain = {}

    def group(self, lo, n_frames, kind='frames'):
        f = self.faces[6 * lo:6 * (lo + n_frames)]
        if kind == 'zeros':
            return torch.zeros_like(f)
        return (f * 24.0).contiguous() if kind == 'large' else f.contiguous()

    def plain(self, lo, n_frames):
        """cp360_resnet_forward on frames [lo, lo + n_frames) alone (computed once, never written again)."""
        key = (lo, n_frames)
        if key not in self._plain:
            with torch.no_grad():
                cam, _ = self.stage.forward(self.group(lo, n_frames), want_feat=False)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(cam).all()) and float(cam.abs().max()) > 0
            self._plain[key] = cam.clone()
        return self._plain[key]

    def multi(self, groups):
        n = groups[0].shape[0]
        out = torch.full((len(groups), n, HW, HW, NC), float('nan'), dtype=torch.float32, device='cuda')
        with torch.no_grad():
            got = self.stage.forward_multi(groups, out)
        torch.cuda.synchronize()
        return got


@pytest.fixture(scope='module', params=['fp16', 'bf16'])
def net(request, resnet_state):
    return _Net(resnet_state, request.param)


def test_two_groups_of_one_cube_equal_the_plain_forward(net):
    """Two groups of 6 faces (one cube each): every group's CAM is cp360_resnet_forward's on that group alone."""
    assert net.stage.can_pair_static(6, CD)
    got = net.multi([net.group(0, 1), net.group(1, 1)])
    assert torch.equal(got[0], net.plain(0, 1)) and torch.equal(got[1], net.plain(1, 1))
    assert not torch.equal(got[0], got[1])
    text = net.stage.describe_multi(2, 6, CD)
    assert 'FRONT' in text and 'CUT' in text and 'BACK' in text and 'layer3.1' in text.split('CUT')[1]


@pytest.mark.parametrize('swap', [False, True])
def test_a_group_does_not_see_its_partner(net, swap):
    """Two groups of 12 faces: cubes of different frames and the group boundary sit next to each other in the joint buffers.
    One group's CAM is the same bits beside zeros, beside ordinary frames and beside large-valued frames - and the plain
    forward's; the same with the groups swapped."""
    mine, want = net.group(2, 2), net.plain(2, 2)
    for kind in ('zeros', 'frames', 'large'):
        other = net.group(4, 2, kind)
        got = net.multi([other, mine] if swap else [mine, other])
        assert torch.equal(got[1 if swap else 0], want), kind
        if kind == 'frames':
            assert torch.equal(got[0 if swap else 1], net.plain(4, 2))


def _raw(net, faces, cams, ws, nbytes=None, n_groups=None, wp=None):
    L = _lib.lib()
    G = len(faces) if n_groups is None else n_groups
    arr = lambda ps: (C.c_void_p * len(ps))(*ps)
    return L.cp360_resnet_forward_multi(net.h, arr([f.data_ptr() for f in faces]), G, faces[0].shape[0], CD, arr(cams),
                                        C.c_void_p(ws.data_ptr() if wp is None else wp), ws.numel() if nbytes is None else nbytes,
                                        _lib.stream())


def test_one_group_is_the_plain_forward_and_a_split_cam_buffer_is_refused(net):
    L = _lib.lib()
    f0, f1 = net.group(0, 1), net.group(1, 1)
    per = 6 * HW * HW * NC
    assert L.cp360_resnet_forward_multi_workspace_bytes(net.h, 1, 6, CD) == L.cp360_resnet_workspace_bytes(net.h, 6, CD)
    assert not net.stage.can_pair_static(6, CD, groups=1)
    got = net.multi([f0])
    assert torch.equal(got[0], net.plain(0, 1))
    # cam_out[1] must follow cam_out[0] directly: anything else is CP360_ERR_BAD_SHAPE before any launch
    nb = L.cp360_resnet_forward_multi_workspace_bytes(net.h, 2, 6, CD)
    ws = torch.empty(nb, dtype=torch.uint8, device='cuda')
    cam = torch.full((3 * per,), -7.0, dtype=torch.float32, device='cuda')
    base = cam.data_ptr()
    assert _raw(net, [f0, f1], [base, base + 4 * (per + 16)], ws) == -1
    assert _raw(net, [f0, f1], [base + 4 * per, base], ws) == -1
    assert _raw(net, [f0, f1], [base, None], ws) == -5
    torch.cuda.synchronize()
    assert bool((cam == -7.0).all())
    assert _raw(net, [f0, f1], [base, base + 4 * per], ws) == 0
    torch.cuda.synchronize()
    assert torch.equal(cam[:per].view(6, HW, HW, NC), net.plain(0, 1)) and torch.equal(cam[per:2 * per].view(6, HW, HW, NC), net.plain(1, 1))
    assert bool((cam[2 * per:] == -7.0).all())


def test_workspace_size_and_alignment(net):
    L = _lib.lib()
    f0, f1 = net.group(0, 1), net.group(1, 1)
    per = 6 * HW * HW * NC
    nb = L.cp360_resnet_forward_multi_workspace_bytes(net.h, 2, 6, CD)
    assert nb % 256 == 0
    # the four activation slots and the scratch of one batch + the hand-over buffer [2 * 6, 14, 14, 1024]
    assert nb >= L.cp360_resnet_workspace_bytes(net.h, 6, CD) + 2 * 6 * 14 * 14 * 1024 * 2
    assert L.cp360_resnet_forward_multi_workspace_bytes(net.h, 0, 6, CD) == 0
    assert L.cp360_resnet_forward_multi_workspace_bytes(net.h, 5, 6, CD) == 0
    assert L.cp360_resnet_forward_multi_workspace_bytes(net.h, 2, 5, CD) == 0
    assert L.cp360_resnet_forward_multi_workspace_bytes(None, 2, 6, CD) == 0
    ws = torch.empty(nb + 256, dtype=torch.uint8, device='cuda')
    assert ws.data_ptr() % 256 == 0
    cam = torch.full((2 * per,), -7.0, dtype=torch.float32, device='cuda')
    cams = [cam.data_ptr(), cam.data_ptr() + 4 * per]
    assert _raw(net, [f0, f1], cams, ws, nbytes=nb - 1) == -1
    assert _raw(net, [f0, f1], cams, ws, nbytes=nb, wp=ws.data_ptr() + 16) == -6
    torch.cuda.synchronize()
    assert bool((cam == -7.0).all())
    assert _raw(net, [f0, f1], cams, ws, nbytes=nb) == 0                      # exactly the queried size is enough
    torch.cuda.synchronize()
    assert torch.equal(cam[per:].view(6, HW, HW, NC), net.plain(1, 1))


# ------------------------------------------------------------------ the engine
@pytest.fixture(scope='module')
def clstm_state():
    return synth.clstm_state(seed=3)


def _batches(B, T, k0, n):
    return [torch.from_numpy(np.stack([synth.clip_u8(k0 + B * k + b, T, H, W) for b in range(B)])).cuda() for k in range(n)]


def test_stream_pairs_the_static_back_half_with_the_same_bits(resnet_state, clstm_state, monkeypatch):
    """4 clips x 2 frames (the ConvLSTM pairs on the Winograd plan, the static stage at cube 224 in fp16), 3 distinct batches: one
    joint static call for batches 0 and 1, the plain one for the last batch, and every map equals __call__'s."""
    from cp_360_weakly_supervised_saliency_amd.pipeline import SaliencyEngine
    B, T = 4, 2
    clips = _batches(B, T, 80, 3)
    eng = SaliencyEngine(resnet_state, clstm_state, (H, W), CD, clips=B, frames=T, precision='bf16')
    try:
        want = [eng(c).clone() for c in clips]
        assert eng.pair.can_pair() and eng.can_pair_static()
        calls = {'multi': 0, 'plain': 0}
        m0, p0 = stage_ctx.ResnetStage.forward_multi, stage_ctx.ResnetStage.forward

        def multi(stage, *a, **k):
            calls['multi'] += 1
            return m0(stage, *a, **k)

        def plain(stage, *a, **k):
            calls['plain'] += 1
            return p0(stage, *a, **k)
        monkeypatch.setattr(stage_ctx.ResnetStage, 'forward_multi', multi)
        monkeypatch.setattr(stage_ctx.ResnetStage, 'forward', plain)
        got = [m.clone() for m in eng.stream(iter(clips))]
        assert calls == {'multi': 1, 'plain': 1}
        assert len(got) == 3
        for k, (a, b) in enumerate(zip(got, want)):
            assert bool(torch.isfinite(b).all()) and torch.equal(a, b), k
        assert not torch.equal(want[0], want[1]) and not torch.equal(want[1], want[2])
        assert torch.equal(eng(clips[1]), want[1])                            # __call__ after the stream: the CAM buffers moved, the bits did not
        assert eng._batch == 7 and not eng.overflow_batches
        eng.check()
    finally:
        eng.close()


@pytest.mark.parametrize('prec,cube', [('fp32', 224), ('bf16', 256)])
def test_engines_that_cannot_pair_the_static_stage_stream_as_before(resnet_state, clstm_state, prec, cube):
    """f32 and cube 256 have no joint back half: can_pair_static is False and the stream still equals __call__."""
    from cp_360_weakly_supervised_saliency_amd.pipeline import SaliencyEngine
    B, T = 1, 2
    clips = _batches(B, T, 95, 3)
    eng = SaliencyEngine(resnet_state, clstm_state, (H, W), cube, clips=B, frames=T, precision=prec)
    try:
        want = [eng(c).clone() for c in clips]
        assert not eng.can_pair_static()
        got = [m.clone() for m in eng.stream(iter(clips))]
        assert len(got) == 3
        for k, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(a, b), (prec, cube, k)
    finally:
        eng.close()
