"""BASELINE.json configs C2 / C3 / C4 at the resolution they are quoted on (1024x2048 equirectangular,
cube 224), HIP path vs the oracle:

  C2  1 frame, fp32, static path only (equi -> cube -> CubePad ResNet-50 -> CAM):
      window-normalised CAM within 1e-3.
  C3  one 16-frame clip, bf16 (and fp32: saliency within 1e-3 abs).
  C4  the per-GPU shard of config C4: 4 clips x 16 frames batched through one engine, bf16 -
      every clip against the oracle run on that clip alone.

"bf16" is the engine's default 16-bit mode: ConvLSTM (81 % of the flops) in bf16, static stage in fp16 (same
MFMA rate; a bf16 ResNet alone moves the map by 3.4e-3 and CC by 1.2e-3, tests/probe_precision_split.py).
The all-bf16 engine (static_precision='bf16') is run too, against the looser bound it actually meets.

The 16-bit gate follows SURVEY 8(d): AUC-Judd and CC of the build's map against a fixation map
within 1e-3 of the same metrics of the oracle's map - with fixations SAMPLED FROM THE ORACLE MAP
(synth.fixations_from_map), so the oracle scores well above chance and a wrong map cannot pass by
both being at chance level - and additionally CC(build, oracle) >= 0.9999.
Follows /root/reference/temporal_model/test_temporal.py:57-110 (window, c2e, metrics).
"""
import numpy as np
import pytest
import torch

from oracle import o_metrics
from cp_360_weakly_supervised_saliency_amd.utils import synth
from tests import parity_helpers as ph

pytestmark = pytest.mark.gpu

H, W, CD, T, B = 1024, 2048, 224, 16, 4


def _metrics(m, fix):
    return (o_metrics.auc_judd(m, fix, rng=np.random.RandomState(0)), o_metrics.corr_coeff(m, fix))


def gate_16bit(sal, ref, seed, label, dcc=1e-3):
    """|dAUC-Judd| <= 1e-3, |dCC| <= 1e-3 (``dcc``) against oracle-correlated fixations, CC(build, oracle) >= 0.9999."""
    fix = synth.fixations_from_map(ref, seed, H // 2, W // 2)
    auc_r, cc_r = _metrics(ref, fix)
    auc, cc = _metrics(sal, fix)
    cc_bo = o_metrics.corr_coeff(sal, ref)
    print('%s: oracle AUC-Judd %.4f CC %.4f | dAUC %+.2e dCC %+.2e CC(build,oracle) %.6f max|d| %.2e'
          % (label, auc_r, cc_r, auc - auc_r, cc - cc_r, cc_bo, float(np.max(np.abs(sal - ref)))))
    assert auc_r > 0.7 and cc_r > 0.1, "fixations must be informative for the oracle map"
    assert abs(auc - auc_r) <= 1e-3, (label, auc, auc_r)
    assert abs(cc - cc_r) <= dcc, (label, cc, cc_r)
    assert cc_bo >= 0.9999, (label, cc_bo)


@pytest.fixture(scope='module')
def shard():
    """4 clips x 16 frames of 1024x2048 and the oracle's result for each clip (64 oracle frames)."""
    rs = synth.resnet50_state(seed=1)
    cs = synth.clstm_state(seed=2)
    clips = np.stack([synth.clip_u8(3 + b, T, H, W) for b in range(B)])          # bench.py's clips of rank 0
    refs = [ph.oracle_pipeline(clips[b], rs, cs, CD, return_all=True) for b in range(B)]
    return dict(rs=rs, cs=cs, clips=clips, refs=refs)


def test_c2_one_frame_fp32_static(shard):
    from cp_360_weakly_supervised_saliency_amd.pipeline import SaliencyEngine
    s = shard
    eng = SaliencyEngine(s['rs'], s['cs'], (H, W), CD, clips=1, frames=1, precision='fp32')
    frame = torch.from_numpy(s['clips'][0, :1]).cuda()
    with torch.no_grad():
        cam = eng.static_stage(frame).cpu().numpy()[0, 0]                        # [294, 1000] NHWC
    want = s['refs'][0][1][0].transpose(0, 2, 3, 1).reshape(294, 1000)          # oracle frame 0 [6,1000,7,7]
    mn, mx = want.min(), want.max()
    err = np.max(np.abs((cam - mn) / (mx - mn) - (want - mn) / (mx - mn)))
    print('C2 fp32 window-normalised CAM max|d| %.2e, relative %.2e' % (err, np.max(np.abs(cam - want)) / np.max(np.abs(want))))
    assert err <= 1e-3
    assert np.max(np.abs(cam - want)) <= 1e-4 * np.max(np.abs(want))


@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
def test_c3_one_clip_16_frames(shard, prec):
    from cp_360_weakly_supervised_saliency_amd.pipeline import SaliencyEngine
    s = shard
    eng = SaliencyEngine(s['rs'], s['cs'], (H, W), CD, clips=1, frames=T, precision=prec)
    sal = eng(torch.from_numpy(s['clips'][:1]).cuda()).cpu().numpy()[0]
    ref = s['refs'][0][0]
    assert sal.shape == ref.shape == (14, 28)
    if prec == 'fp32':
        assert np.max(np.abs(sal - ref)) <= 1e-3                                  # the north-star fp32 bound
    gate_16bit(sal, ref, 200, 'C3 %s' % prec)


def gate_all_bf16(sal, ref, seed, label):
    """The bounds the all-bf16 engine meets: |dAUC-Judd| <= 1e-3, |dCC| <= 3e-3, CC(build, oracle) >= 0.9995, max|d| <= 1e-2."""
    fix = synth.fixations_from_map(ref, seed, H // 2, W // 2)
    (auc_r, cc_r), (auc, cc) = _metrics(ref, fix), _metrics(sal, fix)
    print('%s: dAUC %+.2e dCC %+.2e CC(build,oracle) %.6f max|d| %.2e'
          % (label, auc - auc_r, cc - cc_r, o_metrics.corr_coeff(sal, ref), float(np.max(np.abs(sal - ref)))))
    assert abs(auc - auc_r) <= 1e-3 and abs(cc - cc_r) <= 3e-3, (label, auc - auc_r, cc - cc_r)
    assert o_metrics.corr_coeff(sal, ref) >= 0.9995 and np.max(np.abs(sal - ref)) <= 1e-2, label


def test_c3_all_bf16_static_stage_too(shard):
    """bf16 in BOTH stages (not the default): the bf16 ResNet moves the map ~8x more than fp16 does; it
    stays within 1e-3 on AUC-Judd but not on CC - recorded here with the bounds it meets."""
    from cp_360_weakly_supervised_saliency_amd.pipeline import SaliencyEngine
    s = shard
    eng = SaliencyEngine(s['rs'], s['cs'], (H, W), CD, clips=1, frames=T, precision='bf16', static_precision='bf16')
    sal = eng(torch.from_numpy(s['clips'][:1]).cuda()).cpu().numpy()[0]
    gate_all_bf16(sal, s['refs'][0][0], 200, 'C3 all-bf16')


@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
def test_c4_shard_4_clips_x_16_frames_batched(shard, prec):
    from cp_360_weakly_supervised_saliency_amd.pipeline import SaliencyEngine
    s = shard
    eng = SaliencyEngine(s['rs'], s['cs'], (H, W), CD, clips=B, frames=T, precision=prec)
    sal = eng(torch.from_numpy(s['clips']).cuda()).cpu().numpy()
    assert sal.shape == (B, 14, 28)
    for b in range(B):
        ref = s['refs'][b][0]
        if prec == 'fp32':
            assert np.max(np.abs(sal[b] - ref)) <= 1e-3, b
        gate_16bit(sal[b], ref, 210 + b, 'C4 shard %s clip %d' % (prec, b))
    if prec == 'fp32':
        # the static stage of the whole shard (64 frames batched): window-normalised CAM per clip
        cam = eng.cam.cpu().numpy()                                               # [B, T, 294, 1000]
        for b in range(B):
            want = s['refs'][b][1].transpose(0, 1, 3, 4, 2).reshape(T, 294, 1000)
            mn, mx = want.min(), want.max()
            assert np.max(np.abs((cam[b] - mn) / (mx - mn) - (want - mn) / (mx - mn))) <= 1e-3, b


@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
def test_c2_variant_cube_256_pipeline(prec):
    """SURVEY 8, "C2 ... cd=256 optional variant" (the reference's only smoke test uses 256-pixel faces, model/cube_pad.py:256-261):
    a 1024x2048 clip through cube 256 -> layer4 8x8 -> ConvLSTM at 8x8 faces -> 16x32 map, against the oracle end to end.
    None of the fused static-stage kernels is specialised to this geometry: the static stage takes the per-convolution path
    (cp360_resnet_plan_describe says so).  The ConvLSTM of ONE clip at 8x8 faces runs the HALF variant of the clip-resident kernel
    (conv_clip_kernel<T, 2>: half a cube per tile, the whole cube resident); four clips would run in the Winograd domain
    (tests/test_wino.py::test_wino_cell_window_matches_oracle[bf16-8-4])."""
    from cp_360_weakly_supervised_saliency_amd.pipeline import SaliencyEngine
    cd, t = 256, 3
    rs = synth.resnet50_state(seed=1)
    cs = synth.clstm_state(seed=2)
    clip = synth.clip_u8(41, t, H, W)
    ref = ph.oracle_pipeline(clip, rs, cs, cd)
    eng = SaliencyEngine(rs, cs, (H, W), cd, clips=1, frames=t, precision=prec)
    sal = eng(torch.from_numpy(clip[None]).cuda()).cpu().numpy()[0]
    assert sal.shape == ref.shape == (16, 32)
    err = float(np.max(np.abs(sal - ref)))
    print('cube 256 %s: map max|d| %.2e, CC(build, oracle) %.6f' % (prec, err, o_metrics.corr_coeff(sal, ref)))
    if prec == 'fp32':
        assert err <= 1e-3                                                        # the north-star fp32 bound
    else:
        assert err <= 5e-3 and o_metrics.corr_coeff(sal, ref) >= 0.9999
    from cp_360_weakly_supervised_saliency_amd import stage_ctx
    if stage_ctx.USE_CTX:                                                          # (CP360_CTX=0 plans in Python: no context to ask)
        plan = eng.resnet.__dict__['_stage'].describe(6 * t, cd)
        assert 'layer1: GENERIC path' in plan and 'layer3.1-5: GENERIC path' in plan


# ------------------------------------------------------------------ the launch shapes bench.py times, layer by layer
# (faces, cube, static-stage dtype): C4 headline / sustained (fp16 static stage of the bf16 engine), the all-bf16 secondary,
# the cube-256 variant (generic path) - all 4 clips x 16 frames - and C5 (one 16-frame clip at cube 512)
BENCH_STATIC_SHAPES = [(384, 224, 'fp16'), (384, 224, 'bf16'), (384, 256, 'fp16'), (96, 512, 'fp16')]
_LAYERS = ['stem', 'layer1', 'layer2', 'layer3', 'layer4.0', 'layer4.1', 'layer4.2', 'cam']


def _assert_static_paths(plan, cd):
    """Which path every layer takes at this shape (cp360_resnet_plan_describe), so that a planner change cannot move a layer
    off the path the per-layer check believes it covers."""
    if cd == 224:
        want = ['stem: FUSED stem', 'layer1: ONE fused launch per Bottleneck', 'layer2.0: ONE fused launch',
                'layer2.1-3: conv1 + ONE fused tail launch', 'layer3.0: generic path', 'layer3.1-5: conv1 + ONE fused tail launch']
        assert 'GENERIC' not in plan, plan
    elif cd == 512:
        want = ['stem: resident-patch stem kernel', 'layer1: conv1 of block 0, then ONE fused launch', 'layer2.0: generic path',
                'layer2.1-3: conv1 + ONE fused tail launch', 'layer3.0: generic path', 'layer3.1-5: conv1 + ONE fused tail launch']
        assert 'GENERIC' not in plan, plan
    else:
        want = ['stem: generic convolution', 'layer1: GENERIC path', 'layer2.0: generic path', 'layer2.1-3: GENERIC path',
                'layer3.0: generic path', 'layer3.1-5: GENERIC path']
    want += ['layer4: one launch per convolution', 'CAM: 1x1 convolution']
    for w in want:
        assert w in plan, (w, plan)


@pytest.mark.parametrize('n_img,cd,prec', BENCH_STATIC_SHAPES)
def test_static_stage_per_layer_at_bench_shapes(shard, n_img, cd, prec):
    """The 16-bit static stage at the batch bench.py times, one layer at a time (stem + pool, layer1-3, each layer4 block, the
    CAM conv), against torch-CPU f32 from the GPU's own rounded input to that layer.  The GPU runs every face of the batch
    (real frames of the shard through Equi2Cube), so tiles, split-K and the persistent loops are the timed ones; the CPU
    recomputes 8 sampled cubes.  Per-face bound: tests/parity_helpers.TOL x the layer factor of the fused-kernel tests.
    Each check is shown to reject its own output with one band of one face moved by 4x its bound."""
    from cp_360_weakly_supervised_saliency_amd import stage_ctx
    from cp_360_weakly_supervised_saliency_amd.model.resnet_cubic import resnet50
    from cp_360_weakly_supervised_saliency_amd.utils.equi_to_cube import Equi2Cube
    s = shard
    dt = {'fp16': torch.float16, 'bf16': torch.bfloat16}[prec]
    m = resnet50(precision=prec)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in s['rs'].items()}, strict=False)
    m = m.cuda().eval()
    st = stage_ctx.ResnetStage(m)
    plan = st.describe(n_img, cd)
    st.close()
    print(plan)
    _assert_static_paths(plan, cd)
    frames = s['clips'].reshape((B * T,) + s['clips'].shape[2:])[:n_img // 6]
    with torch.no_grad():
        xp = Equi2Cube(cd, (H, W), device='cuda').to_cube_batch(torch.from_numpy(frames).cuda(), out_dtype=dt, layout='nhwc4p3')
    assert tuple(xp.shape) == (n_img, cd + 6, cd + 6, 4)
    cubes = ph.sample_cubes(n_img // 6)
    trace = ph.static_layer_trace(m, xp, cubes)
    del xp, m, st
    torch.cuda.empty_cache()
    want = ph.static_layer_reference(trace, s['rs'], prec)
    fails = []
    for name in _LAYERS:
        bound = ph.TOL[prec] * ph.LAYER_FACTOR[name]
        got = trace[name].numpy()
        assert np.isfinite(got).all(), name
        err, _, msg = ph.per_face_error(got, want[name], bound, '%s %d x %d^2 %s' % (name, n_img, cd, prec), cubes)
        print('%d faces of %d^2 %s %-9s worst per-face error %.3e (bound %.3e)' % (n_img, cd, prec, name, err, bound))
        if err > bound:
            fails.append(msg)
        # the check rejects a band of 7 rows x 64 channels of one face of the last sampled cube moved by 4x its bound
        bad = ph.perturb_band(got, want[name], bound, 6 * len(cubes) - 3)
        assert ph.per_face_error(bad, want[name], bound, name, cubes)[0] > bound, name
    assert not fails, '\n'.join(fails)


# window-normalised CAM of the whole C4 shard against the oracle, per frame and face: bound <= 2x the worst value measured on an
# MI355X (fp16 static stage of the bf16 engine: 3.03e-3, median over the 384 faces 2.0e-3; all-bf16: 2.52e-2, median 1.8e-2)
CAM_BOUND = {'fp16': 6e-3, 'bf16': 5e-2}


@pytest.mark.parametrize('sprec', ['fp16', 'bf16'])
def test_c4_shard_16bit_cam_per_frame_and_face(shard, sprec):
    """The 16-bit CAM of every frame of the 4 x 16 shard (the headline's static stage: 384 faces in one batch) against the
    oracle's, window-normalised with the oracle's clip min / max, max|d| per frame and face.  The map-level gate (gate_16bit)
    reduces all of it to 392 numbers after 16 ConvLSTM steps; this bounds every face of every frame.  Measured on an MI355X:
    worst 3.03e-3 with the fp16 static stage (clip 3 frame 0 face 2), 2.52e-2 all-bf16 (clip 1 frame 6 face 0)."""
    from cp_360_weakly_supervised_saliency_amd.pipeline import SaliencyEngine
    s = shard
    eng = SaliencyEngine(s['rs'], s['cs'], (H, W), CD, clips=B, frames=T, precision='bf16',
                         static_precision=None if sprec == 'fp16' else 'bf16')
    eng(torch.from_numpy(s['clips']).cuda())
    assert eng.static_precision == sprec and not eng.fp16_fallback
    cam = eng.cam.cpu().numpy().reshape(B, T, 6, 49, 1000)
    bound = CAM_BOUND[sprec]
    errs = np.zeros((B, T, 6))
    win = []
    for b in range(B):
        want = s['refs'][b][1].transpose(0, 1, 3, 4, 2).reshape(T, 6, 49, 1000)
        mn, mx = float(want.min()), float(want.max())
        win.append((mn, mx))
        errs[b] = np.abs(cam[b] - want).max(axis=(2, 3)) / (mx - mn)
    b, t, f = np.unravel_index(int(np.argmax(errs)), errs.shape)
    print('C4 shard %s CAM: window-normalised max|d| per frame and face: worst %.3e (clip %d frame %d face %d), median %.3e, '
          'bound %.3e' % (sprec, errs.max(), b, t, f, np.median(errs), bound))
    assert errs.max() <= bound, (errs.max(), b, t, f)
    # the check rejects one band (7 rows x 64 channels) of one face of the last frame of the last clip moved by 4x the bound
    # (in window units: the metric's own scale)
    b, t, f = B - 1, T - 1, 3
    mn, mx = win[b]
    delta = 4.0 * bound * (mx - mn)
    want = s['refs'][b][1][t, f].transpose(1, 2, 0)                              # [7, 7, 1000]
    bad = cam[b, t, f].reshape(7, 7, 1000).copy()
    bad[:, :, 468:532] += delta
    assert np.abs(bad - want).max() / (mx - mn) > bound
    # ... which the map-level gate does not necessarily see: the same perturbation written into the CAM the ConvLSTM reads
    eng.cam.view(B, T, 6, 7, 7, 1000)[b, t, f, :, :, 468:532] += delta
    sal_bad = eng.temporal_stage().cpu().numpy()[b]
    try:
        gate_16bit(sal_bad, s['refs'][b][0], 210 + b, 'C4 shard %s clip %d, perturbed CAM' % (sprec, b))
        seen = 'passes'
    except AssertionError:
        seen = 'rejects it'
    print('gate_16bit on the map of the perturbed CAM: %s' % seen)
    del eng
    torch.cuda.empty_cache()


def test_c4_all_bf16_4_clips_x_16_frames(shard):
    """The all-bf16 secondary line (static stage bf16 too) at its timed shape, every clip against the oracle with the bounds
    test_c3_all_bf16_static_stage_too meets."""
    from cp_360_weakly_supervised_saliency_amd.pipeline import SaliencyEngine
    s = shard
    eng = SaliencyEngine(s['rs'], s['cs'], (H, W), CD, clips=B, frames=T, precision='bf16', static_precision='bf16')
    sal = eng(torch.from_numpy(s['clips']).cuda()).cpu().numpy()
    for b in range(B):
        gate_all_bf16(sal[b], s['refs'][b][0], 210 + b, 'C4 all-bf16 clip %d' % b)
    del eng
    torch.cuda.empty_cache()


def test_cube_256_variant_4_clips_x_16_frames(shard):
    """The cube-256 secondary line at its timed shape (bf16 engine, 384 faces of 256^2 on the generic static path, the ConvLSTM
    in the Winograd domain at 8x8 faces), clips 0 and 3 against the oracle (clips are independent) with the 16-bit bounds of
    test_c2_variant_cube_256_pipeline."""
    from cp_360_weakly_supervised_saliency_amd.pipeline import SaliencyEngine
    s = shard
    cd = 256
    eng = SaliencyEngine(s['rs'], s['cs'], (H, W), cd, clips=B, frames=T, precision='bf16')
    sal = eng(torch.from_numpy(s['clips']).cuda()).cpu().numpy()
    assert sal.shape == (B, 16, 32)
    assert eng.cell.uses_winograd(6 * B, eng.w)
    from cp_360_weakly_supervised_saliency_amd import stage_ctx
    if stage_ctx.USE_CTX:
        plan = eng.resnet.__dict__['_stage'].describe(6 * B * T, cd)
        assert 'layer1: GENERIC path' in plan and 'layer3.1-5: GENERIC path' in plan
    del eng
    torch.cuda.empty_cache()
    for b in (0, B - 1):
        ref = ph.oracle_pipeline(s['clips'][b], s['rs'], s['cs'], cd)
        err = float(np.max(np.abs(sal[b] - ref)))
        cc = o_metrics.corr_coeff(sal[b], ref)
        print('cube 256 4x16 bf16 clip %d: map max|d| %.2e, CC(build, oracle) %.6f' % (b, err, cc))
        assert err <= 5e-3 and cc >= 0.9999, (b, err, cc)


def test_c4_f32_resident_frames(shard):
    """The f32-input secondary line: frames resident as u8 / 255 in f32 (as bench.py's run_workload(f32_input=True) builds
    them) through the bf16 engine at 4 x 16, against the oracle with the gate of the u8 path."""
    from cp_360_weakly_supervised_saliency_amd.pipeline import SaliencyEngine
    s = shard
    eng = SaliencyEngine(s['rs'], s['cs'], (H, W), CD, clips=B, frames=T, precision='bf16')
    frames = torch.from_numpy(s['clips']).cuda().to(torch.float32) / 255.0
    sal = eng(frames).cpu().numpy()
    del frames, eng
    torch.cuda.empty_cache()
    for b in range(B):
        gate_16bit(sal[b], s['refs'][b][0], 210 + b, 'C4 f32 frames clip %d' % b)


@pytest.fixture(scope='module')
def shard_traces(shard):
    """The oracle's map after every ConvLSTM step of clips 0 and 3, from the shard's CAMs."""
    from oracle import o_clstm, o_c2e
    sdt = ph.sd_t(shard['cs'])
    return {b: np.stack([o_c2e.saliency_from_hidden(h) for h in o_clstm.window_hidden(shard['refs'][b][1], sdt, all_steps=True)])
            for b in (0, B - 1)}


@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
def test_c4_return_all_steps_through_the_engine(shard, shard_traces, prec):
    """The return_all_steps secondary line at 4 x 16: the last step equals the plain engine's map bit for bit, and every step
    of clips 0 and 3 matches the oracle's hidden trace (fp32 within 1e-3, bf16 by the C4 gate per step).  The bf16 gate's
    |dCC| bound is 1e-3 at the last step - the map the C4 test gates - and 2e-3 before it: the bf16 cell in the Winograd domain
    (4 windows) has about twice the map error of the direct kernel (1 window) at every step, and on an MI355X one early map
    (clip 3 step 0: max|d| 1.8e-3, CC(build, oracle) 0.99999) moved |dCC| by 1.16e-3."""
    from cp_360_weakly_supervised_saliency_amd.pipeline import SaliencyEngine
    s = shard
    clips = torch.from_numpy(s['clips']).cuda()
    eng = SaliencyEngine(s['rs'], s['cs'], (H, W), CD, clips=B, frames=T, precision=prec, return_all_steps=True)
    maps = eng(clips).cpu()
    del eng
    torch.cuda.empty_cache()
    eng = SaliencyEngine(s['rs'], s['cs'], (H, W), CD, clips=B, frames=T, precision=prec)
    last = eng(clips).cpu()
    del eng, clips
    torch.cuda.empty_cache()
    assert tuple(maps.shape) == (B, T, 14, 28)
    assert torch.equal(maps[:, T - 1], last)
    maps = maps.numpy()
    for b, trace in shard_traces.items():
        assert np.max(np.abs(trace[T - 1] - s['refs'][b][0])) <= 1e-6          # the trace ends in the shard's oracle map
        for t in range(T):
            if prec == 'fp32':
                assert np.max(np.abs(maps[b, t] - trace[t])) <= 1e-3, (b, t)
            else:
                gate_16bit(maps[b, t], trace[t], 300 + 16 * b + t, 'C4 all steps bf16 clip %d step %d' % (b, t),
                           dcc=1e-3 if t == T - 1 else 2e-3)


def test_c3_graph_replay_equals_eager(shard):
    """The C3 hipGraph secondary line (one 16-frame clip of 1024 x 2048, bf16): replay == eager bit for bit, with other clip
    contents copied in between."""
    from cp_360_weakly_supervised_saliency_amd.pipeline import SaliencyEngine
    s = shard
    eng = SaliencyEngine(s['rs'], s['cs'], (H, W), CD, clips=1, frames=T, precision='bf16')
    a = torch.from_numpy(s['clips'][:1]).cuda()
    b = torch.from_numpy(s['clips'][B - 1:]).cuda()
    eager_a = eng(a).clone()
    eager_b = eng(b).clone()
    assert not torch.equal(eager_a, eager_b)
    a0 = a.clone()
    eng.capture(a)
    assert torch.equal(eng(a), eager_a)
    assert torch.equal(eng(b), eager_b)
    assert torch.equal(eng(a0), eager_a)
    del eng
    torch.cuda.empty_cache()


def test_c2_static_only_graph_replay_equals_eager(shard):
    """The C2 static-only hipGraph secondary line (one frame, fp32; captured as bench.py captures it: the static stage over a
    fixed input buffer): replay == eager bit for bit, with another frame copied in between."""
    from cp_360_weakly_supervised_saliency_amd.pipeline import SaliencyEngine
    s = shard
    eng = SaliencyEngine(s['rs'], s['cs'], (H, W), CD, clips=1, frames=1, precision='fp32')
    fa = torch.from_numpy(s['clips'][0, :1]).cuda()
    fb = torch.from_numpy(s['clips'][B - 1, 5:6]).cuda()
    with torch.no_grad():
        eager_a = eng.static_stage(fa).clone()
        eager_b = eng.static_stage(fb).clone()
        assert not torch.equal(eager_a, eager_b)
        inp = fa.clone()
        eng.static_stage(inp)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            eng.static_stage(inp)
        for f, want in ((fa, eager_a), (fb, eager_b), (fa, eager_a)):
            inp.copy_(f)
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(eng.cam, want)
    del g, eng
    torch.cuda.empty_cache()
