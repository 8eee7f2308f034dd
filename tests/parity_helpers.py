"""Oracle-side compositions shared by the GPU parity tests, smoke() and the
cpu_baseline leg of bench.py.  Imports oracle/ - never imported by the product."""
import numpy as np
import torch

from oracle import o_e2c, o_resnet, o_clstm, o_c2e


def sd_t(sd):
    return {k: (v if torch.is_tensor(v) else torch.from_numpy(v)) for k, v in sd.items()}


def oracle_cubes(frame_u8, cube_dim, grids=None, fixed_point=True):
    """dataset_feat_extractor.py:138-157: u8 frame -> /255 (float64) -> to_cube ->
    im_norm -> float32 [6, 3, cd, cd]."""
    img = np.array(frame_u8) / 255.0
    cubes = o_e2c.to_cube(img, cube_dim, fixed_point=fixed_point, grids=grids)
    return o_e2c.im_norm_batch(cubes)


def oracle_cam_frames(clip_u8, resnet_sd, cube_dim):
    """[T, H, W, 3] u8 -> cube_feat [T, 6, 1000, h, w] float32 (static stage)."""
    sd = sd_t(resnet_sd)
    H, W = clip_u8.shape[1:3]
    grids = o_e2c.grids_f32(cube_dim, H, W)
    out = []
    for t in range(clip_u8.shape[0]):
        score, _ = o_resnet.cam_from_cubes(oracle_cubes(clip_u8[t], cube_dim, grids), sd)
        out.append(score.astype(np.float32))
    return np.stack(out)


def oracle_pipeline(clip_u8, resnet_sd, clstm_sd, cube_dim, align_corners=False, return_all=False):
    """One clip = one window: frames -> saliency [2w, 4w] float32."""
    cams = oracle_cam_frames(clip_u8, resnet_sd, cube_dim)
    hid = o_clstm.window_hidden(cams, sd_t(clstm_sd))
    sal = o_c2e.saliency_from_hidden(hid, align_corners=align_corners)
    return (sal, cams, hid) if return_all else sal


def cubepad_sweep(dev):
    """Seeded geometry sweep of the stand-alone NCHW CubePad against the oracle (see
    tests/test_gpu_parity.py::test_cubepad_nchw_randomised_geometry_sweep)."""
    from oracle import o_cubepad
    from cp_360_weakly_supervised_saliency_amd.model.cube_pad import CubePad
    rng = np.random.RandomState(20260)
    dts = [torch.uint8, torch.int16, torch.int32, torch.int64]
    npd = {torch.uint8: np.uint8, torch.int16: np.int16, torch.int32: np.int32, torch.int64: np.int64}
    cases = []
    for _ in range(60):
        n = int(rng.choice([1, 2, 3, 5, 7, 8, 14, 16, 28, 31, 32, 33, 56, 57, 64, 112, 113, 130]))
        pad = [int(min(n, v)) for v in rng.randint(0, 5, size=4)]
        C = int(rng.randint(1, 24))
        n6 = 6 * int(rng.randint(1, 3))
        dt = dts[int(rng.randint(0, 4))]
        off = int(rng.randint(0, 4))
        cases.append((n, pad, C, n6, dt, off))
    cases += [(56, [1, 1, 1, 1], 64, 12, torch.int16, 0), (57, [2, 0, 1, 3], 50, 12, torch.int16, 1),
              (112, [1, 1, 1, 1], 48, 12, torch.int16, 0), (113, [3, 3, 3, 3], 17, 36, torch.int32, 0),
              (224, [3, 3, 3, 3], 3, 192, torch.int32, 0), (130, [0, 4, 2, 0], 25, 24, torch.uint8, 3),
              (40, [1, 2, 0, 1], 33, 18, torch.int64, 0), (64, [4, 4, 4, 4], 16, 36, torch.int32, 2),
              (256, [1, 1, 1, 1], 16, 36, torch.int16, 0), (28, [1, 1, 1, 1], 128, 24, torch.int16, 0),
              (14, [1, 1, 1, 1], 256, 12, torch.int16, 0), (7, [1, 1, 1, 1], 500, 12, torch.int32, 0),
              (120, [1, 1, 1, 1], 32, 12, torch.int16, 0), (200, [2, 1, 0, 3], 20, 24, torch.uint8, 1)]
    # rows of 112-264 bytes with few items, misaligned bases, a pad sum above 16 lines: row bands down to their floor,
    # the element-per-lane kernel below it (rows within one wave and longer)
    cases += [(120, [1, 1, 1, 1], 2, 6, torch.int16, 1), (60, [2, 1, 0, 3], 3, 6, torch.int32, 0),
              (28, [1, 1, 1, 1], 5, 6, torch.int32, 1), (27, [1, 1, 1, 1], 5, 6, torch.int32, 1),
              (128, [5, 4, 5, 4], 2, 6, torch.int16, 0), (170, [1, 0, 3, 2], 2, 6, torch.uint8, 3),
              (33, [1, 1, 1, 1], 3, 6, torch.int64, 0)]
    for case, (n, pad, C, n6, dt, off) in enumerate(cases):
        x = rng.randint(0, 120, size=(n6, C, n, n)).astype(npd[dt])
        buf = torch.zeros(x.size + off, dtype=dt, device=dev)
        buf[off:] = torch.from_numpy(x).reshape(-1).to(dev)
        want = o_cubepad.cubepad(x, pad)
        got = CubePad(pad)(buf[off:].view(n6, C, n, n)).cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got, want), (case, n, pad, C, n6, dt, off)


# ------------------------------------------------------------------ per-layer parity of the 16-bit static stage
# one output rounding: 2^-8 relative for bf16, 2^-11 for fp16 (tests/test_gpu_parity.py::_TOL)
TOL = {'fp32': 2e-5, 'bf16': 1.2e-2, 'fp16': 1.5e-3}
# bound factor per layer, as the fused-kernel tests of tests/test_gpu_parity.py use them against torch-CPU in f32: the stem
# against rounded weights (test_stem_resident_patch_kernel_cube224), a whole layer of 3-4 blocks x4, layer3 (6 blocks) x6, one
# Bottleneck x2 (test_layer2_first_block_fused_kernel), the CAM one 1x1 convolution
LAYER_FACTOR = {'stem': 1, 'layer1': 4, 'layer2': 4, 'layer3': 6, 'layer4.0': 2, 'layer4.1': 2, 'layer4.2': 2, 'cam': 1}


def sample_cubes(n_cubes, seed=0):
    """The cubes a per-layer check recomputes on the CPU: 0, 1, the middle one, the last two and 3 seeded random ones
    (whole cubes: CubePad reads across the faces of a cube).  Sorted; the last one is the last cube of the batch."""
    fixed = sorted({0, 1, n_cubes // 2, n_cubes - 2, n_cubes - 1})
    rest = [c for c in range(n_cubes) if c not in fixed]
    picks = np.random.RandomState(seed).choice(rest, min(3, len(rest)), replace=False) if rest else []
    return sorted(fixed + [int(c) for c in picks])


def static_layer_trace(model, faces_p3, cubes):
    """The Python-planned static stage (ResNet.features_nhwc's launches, then the CAM conv) one layer at a time on the GPU
    over ALL faces of ``faces_p3`` ([6N, cd+6, cd+6, 4], the model's dtype), so every launch has the real batch's shape.
    Returns {layer: f32 CPU NHWC output of the sampled cubes' faces} (16-bit outputs widened; the CAM's raw f32 scores), with
    'input' = the unpadded 3-channel faces the stem read."""
    from cp_360_weakly_supervised_saliency_amd import ops
    from cp_360_weakly_supervised_saliency_amd.model import resnet_cubic as rc
    faces = torch.tensor([6 * c + f for c in cubes for f in range(6)], device=faces_p3.device)
    take = lambda t: t.index_select(0, faces).float().cpu()
    out = {'input': take(faces_p3[:, 3:-3, 3:-3, :3])}
    with torch.no_grad(), ops.launch_order(rc.LAUNCH_ORDER):
        x = model.stem_nhwc(faces_p3, padded=True)
        out['stem'] = take(x)
        x, mid2 = model.layer1_nhwc(x, want_next=True)
        out['layer1'] = take(x)
        x = model.layer2_nhwc(x, mid2)
        out['layer2'] = take(x)
        x = model.layer3_nhwc(x)
        out['layer3'] = take(x)
        for b, blk in enumerate(model.layer4):
            x = blk.forward_nhwc(x)
            out['layer4.%d' % b] = take(x)
        out['cam'] = take(model.cam_conv().raw_sum_f32(x, None))
    return out


def static_layer_reference(trace, resnet_sd, prec):
    """torch-CPU f32 of every layer of ``static_layer_trace``, each from the GPU's own rounded input to that layer (so a layer
    is checked alone): o_resnet's stem / Bottleneck / CAM arithmetic.  The stem uses the BN-folded weights rounded to the
    16-bit type as the kernels hold them (the bound of its kernel test); the blocks and the CAM use the f32 weights."""
    import torch.nn.functional as Fn
    sd = sd_t(resnet_sd)
    nchw = lambda t: t.permute(0, 3, 1, 2).contiguous()
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
    want = {}
    with torch.no_grad():
        scale = sd['bn1.weight'] / torch.sqrt(sd['bn1.running_var'] + 1e-5)
        bias = sd['bn1.bias'] - sd['bn1.running_mean'] * scale
        w = sd['conv1.weight'] * scale[:, None, None, None]
        if prec != 'fp32':
            w = w.to({'bf16': torch.bfloat16, 'fp16': torch.float16}[prec]).float()
        y = Fn.relu(Fn.conv2d(o_resnet.cubepad_t(nchw(trace['input']), 3), w, bias, stride=2))
        want['stem'] = nhwc(Fn.max_pool2d(o_resnet.cubepad_t(y, 1), 3, 2, 0))
        prev = 'stem'
        for li, nblk in ((1, 3), (2, 4), (3, 6)):
            x = nchw(trace[prev])
            for b in range(nblk):
                x = o_resnet._bottleneck(x, sd, 'layer%d.%d' % (li, b), 2 if (b == 0 and li > 1) else 1, b == 0)
            prev = 'layer%d' % li
            want[prev] = nhwc(x)
        for b in range(3):
            x = o_resnet._bottleneck(nchw(trace[prev]), sd, 'layer4.%d' % b, 2 if b == 0 else 1, b == 0)
            prev = 'layer4.%d' % b
            want[prev] = nhwc(x)
        feat = nchw(trace[prev]).numpy()
        want['cam'] = nhwc(torch.from_numpy(o_resnet.cam_scores(feat, sd['fc.weight'].numpy())))
    return {k: v.numpy() for k, v in want.items()}


def per_face_error(got, want, bound, label, cubes=None):
    """Per-face relative error of f32 NHWC [F, h, w, C] arrays: max|got - want| over a face / max|want| over that face, so one
    bad face cannot hide behind the maximum of the tensor.  -> (worst ratio, per-face ratios, message naming the worst element:
    cube, face, pixel (y, x) and channel; ``cubes`` maps the rows' cube blocks back to batch cube indices)."""
    F = got.shape[0]
    assert got.shape == want.shape, (label, got.shape, want.shape)
    d = np.abs(got - want).reshape(F, -1)
    m = np.maximum(np.abs(want).reshape(F, -1).max(1), 1e-30)
    r = d.max(1) / m
    f = int(np.argmax(r))
    y, x, c = np.unravel_index(int(np.argmax(d[f])), got.shape[1:])
    cube = f // 6 if cubes is None else cubes[f // 6]
    msg = ('%s: per-face max|d| / max|want| = %.3e > bound %.3e at cube %d face %d pixel (%d, %d) channel %d '
           '(got %.6g want %.6g, face max|want| %.4g)' % (label, r[f], bound, cube, f % 6, y, x, c, got[f, y, x, c],
                                                          want[f, y, x, c], m[f]))
    return float(r[f]), r, msg


def perturb_band(got, want, bound, face, rows=7, chans=64):
    """A copy of ``got`` with one band of one face moved by 4 x bound x (that face's max |want|): ``rows`` rows (from the
    middle of the face, all columns) x ``chans`` channels - what a per-face check at ``bound`` must reject."""
    bad = got.copy()
    h, C = got.shape[1], got.shape[3]
    r0 = max(0, h // 2 - rows // 2)
    c0 = max(0, C // 2 - chans // 2)
    bad[face, r0:r0 + rows, :, c0:c0 + chans] += 4.0 * bound * float(np.abs(want[face]).max())
    return bad
