"""Integer numpy restatement of the shot signature (K13, csrc/shots.hip; the specification is DESIGN.md "K13"), of the distance and
of the cut decision, written independently of utils/shots.py, and the synthetic videos the CPU and GPU tests share.

    a_y = floor(cos(phi_y) 1024 + 1/2), phi_y = (1 - (2 y + 1) / H) pi / 2               int [H]
    sig[f, c, b] = sum of a_y over the pixels with frames[f, y, x, c] >> 2 == b           int64 [F, 3, 64], each [f, c, :] sums to T
    sad_t = sum_{c, b} |sig_t - sig_t+1|,  d_t = sad_t / (6 T)                            float64 in [0, 1]
    cut before frame t + 1  <=>  d_t >= thr and d_t >= ratio * median(d_s: 0 < |s - t| <= radius)   (the median of nothing is 0)
"""
import functools

import numpy as np

from cp_360_weakly_supervised_saliency_amd.utils import synth
from tests import stabilize_restate as sr


# ----------------------------------------------------------------------------- the specification
def weights(H):
    """(a int64 [H], their sum).  The latitude as the exact fraction (H - 2 y - 1) / (2 H) of pi."""
    y = np.arange(H, dtype=np.float64)
    a = np.floor(np.cos(np.pi * ((H - 2.0 * y - 1.0) / (2.0 * H))) * 1024.0 + 0.5).astype(np.int64)
    return a, int(a.sum())


def signatures(frames):
    """frames u8 [F, H, W, 3] -> (sig int64 [F, 3, 64], T)."""
    frames = np.asarray(frames)
    assert frames.dtype == np.uint8 and frames.ndim == 4 and frames.shape[3] == 3
    F, H, W, _ = frames.shape
    a, total = weights(H)
    sig = np.zeros((F, 3, 64), np.int64)
    assert W * total < 2 ** 53                                         # bincount sums in float64: exact on integers below 2^53
    wgt = np.repeat(a, W).astype(np.float64)                           # the weight of every pixel, row-major
    for f in range(F):
        for c in range(3):
            bins = (frames[f, :, :, c] >> 2).reshape(-1).astype(np.int64)
            sig[f, c] = np.bincount(bins, weights=wgt, minlength=64).astype(np.int64)
    return sig, W * total


def shot_rows(F, H, W):
    """Rows of a frame per workgroup of K13a: 16 (two per wave) once a video gives the chip F ceil(H / 16) >= 1024 workgroups,
    else 8; halved while a workgroup's u32 partial sums could overflow (R W 1024 > 2^31)."""
    R = 16 if F * -(-H // 16) >= 1024 else 8
    while R > 1 and R * W > 2 ** 21:
        R //= 2
    return R


def work_bytes(F, H, W):
    """cp360_shot_work_bytes: u32 [F, ceil(H / R), 3, 64] partial histograms, to a multiple of 16 bytes.  The size tells which R
    the library chose."""
    return -(-(F * -(-H // shot_rows(F, H, W)) * 192 * 4) // 16) * 16


def sad(sig):
    """sig int64 [F, 3, 64] -> int64 [F - 1]."""
    sig = np.asarray(sig, np.int64)
    return np.abs(sig[1:] - sig[:-1]).reshape(sig.shape[0] - 1, -1).sum(axis=1)


def distances(frames):
    """frames u8 [F, H, W, 3] -> d float64 [F - 1]."""
    sig, T = signatures(frames)
    return sad(sig) / (6 * T)


def find_cuts(d, thr, ratio, radius):
    d = [float(v) for v in np.asarray(d, np.float64).reshape(-1)]
    cuts = []
    for t, v in enumerate(d):
        near = sorted(d[s] for s in range(t - radius, t + radius + 1) if 0 <= s < len(d) and s != t)
        if not near:
            m = 0.0
        elif len(near) % 2:
            m = near[len(near) // 2]
        else:
            m = 0.5 * (near[len(near) // 2 - 1] + near[len(near) // 2])
        if v >= thr and v >= ratio * m:
            cuts.append(t + 1)
    return cuts


def segments(cuts, n):
    out, lo = [], 0
    for c in list(cuts) + [n]:
        out.append((lo, c))
        lo = c
    return out


# ----------------------------------------------------------------------------- the synthetic videos
# (seed of synth.frame_u8, gains, offsets) per channel: three scenes of different tone
SCENES = ((11, (0.9, 0.8, 0.7), (0.05, 0.1, 0.0)),
          (12, (0.5, 0.6, 0.9), (0.4, 0.3, 0.1)),
          (13, (0.6, 0.4, 0.5), (0.0, 0.45, 0.3)))
STEP_DEG = 4.0                                   # the camera turns this much per frame about stabilize_restate.AXIS
THREE_SHOT_LENGTHS = (5, 1, 4)
THREE_SHOT_CUTS = [5, 6]


def toned(values, gains, offsets):
    """values [H, W, 3] in [0, 1] -> u8: value * gain + offset per channel, clipped to [0, 1], rounded."""
    v = np.asarray(values, np.float64) * np.asarray(gains, np.float64) + np.asarray(offsets, np.float64)
    return np.rint(np.clip(v, 0.0, 1.0) * 255.0).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def scene(k, H, W):
    seed, gains, offsets = SCENES[k]
    return toned(synth.frame_u8(seed, H, W) / 255.0, gains, offsets)


def turning(img, n, step_deg=STEP_DEG):
    """n frames of the u8 scene `img`: frame k is the scene under the rotation by k step_deg degrees about AXIS (the float64
    resampler of stabilize_restate, rounded to u8)."""
    R = np.stack([sr.rot(sr.AXIS, np.deg2rad(step_deg * k)) for k in range(n)])
    return sr.equirect_rotate(np.stack([img] * n), R)


@functools.lru_cache(maxsize=None)
def three_shot_video(H, W):
    """u8 [10, H, W, 3]: shots of 5, 1 and 4 frames of the three scenes, each turning 4 degrees per frame; cuts at [5, 6]."""
    return np.concatenate([turning(scene(k, H, W), n) for k, n in enumerate(THREE_SHOT_LENGTHS)])


@functools.lru_cache(maxsize=None)
def two_shot_video(H=64, W=128):
    """For the stabiliser: two shots of 4 frames (3 turns each) of two blurred textures of different tone, the camera turning
    1 - 2 px-equivalents per step as in tests/test_stabilize_gpu.py's moving_camera.  Returns (frames u8 [8, H, W, 3], cut = 4)."""
    px = 2 * np.pi / W
    steps = ([sr.rot(sr.AXIS, 1.5 * px), sr.rot((0.1, 1.0, 0.2), -2.0 * px), sr.rot((1.0, 0.2, -0.3), 1.0 * px)],
             [sr.rot((0.2, -0.5, 1.0), 2.0 * px), sr.rot(sr.AXIS, -1.0 * px), sr.rot((0.0, 1.0, 0.3), 1.5 * px)])
    shots = []
    for k, (seed, st) in enumerate(zip((610, 611), steps)):
        C = [np.eye(3)]
        for s in st:
            C.append(s @ C[-1])
        img = toned(sr.texture(seed, H, W, 3, taps=9), SCENES[k][1], SCENES[k][2])
        shots.append(sr.equirect_rotate(np.stack([img] * 4), np.stack([c.T for c in C])))
    return np.concatenate(shots), 4
