"""Float64 numpy restatement of the anti-aliased view (K21, csrc/viewport.hip: view_pixel_aa; the specification is DESIGN.md
"K21"), on top of tests/viewport_restate.py.

    render_aa  the view (h, w, hfov) under R with the factor n = the n x n box mean of the UNROUNDED samples of K12's view
               (n h, n w, hfov) under the same R: sample (n i + a, n j + b), a, b = 0 .. n - 1 (a along the columns), added with b
               outer and a inner from the first sample, divided by n n; u8 frames round and clamp the quotient
    supersample_for  rho = tan(hfov / 2) max(W, 2 H) / (pi w), the source pixels per view pixel at the view's centre;
               min(limit, max(1, ceil(rho - 1e-9)))

``dtype=np.float32`` evaluates every term in float32 in the kernel's order, as viewport_restate does.  ``render_aa`` takes any
n >= 1: n = 16 is the pixel-box integral the tests measure aliasing against.  Nothing here imports the code under test.
"""
import numpy as np

from tests import stabilize_restate as sr
from tests import viewport_restate as vr


def box_mean(fine, n, dtype=np.float64):
    """fine [N, n h, n w, C] -> [N, h, w, C]: the n x n samples of every pixel added in dtype, b (rows) outer, a (columns) inner,
    starting from the first sample, then divided by dtype(n n)."""
    fine = np.asarray(fine).astype(dtype)
    s = None
    for b in range(n):
        for a in range(n):
            t = fine[:, b::n, a::n]
            s = t.copy() if s is None else s + t
    return s / dtype(n * n)


def render_aa(frames, R, hw, hfov_deg, n, dtype=np.float64, raw=False):
    """frames u8 or float [N, H, W, C], R [N, 3, 3] -> the anti-aliased views [N, h, w, C].  Float frames return dtype; u8 frames
    round half to even and clamp (raw=True: the quotient before rounding, in dtype)."""
    n = int(n)
    if n < 1:
        raise ValueError("n must be at least 1, got %r" % (n,))
    frames = np.asarray(frames)
    fine = vr.render(frames, R, (n * hw[0], n * hw[1]), hfov_deg, dtype, raw=True)
    out = box_mean(fine, n, dtype)
    if frames.dtype == np.uint8 and not raw:
        return np.clip(np.rint(out), 0, 255).astype(np.uint8)
    return out


def rho(HW, hw, hfov_deg):
    """Source pixels per view pixel at the view's centre, float64."""
    return float(np.tan(0.5 * np.deg2rad(float(hfov_deg))) * max(int(HW[1]), 2 * int(HW[0])) / (np.pi * int(hw[1])))


def supersample_for(HW, hw, hfov_deg, limit=4):
    return int(min(int(limit), max(1, int(np.ceil(rho(HW, hw, hfov_deg) - 1e-9)))))


# ----------------------------------------------------------------------------- test inputs shared by the CPU and GPU tests
def cameras4():
    """The four cameras of tests/test_viewport_gpu.py: the identity; a yaw of 180 degrees (the seam inside the view); a pitch of
    90 degrees (centred on the north pole); a generic rotation with roll."""
    return np.stack([np.eye(3), sr.rot((0, 1, 0), np.pi), sr.rot((0, 0, 1), 0.5 * np.pi),
                     sr.rot(sr.AXIS, 1.1) @ sr.rot((1, 0, 0), 0.4)])


# (HW, hw, hfov_deg) with rho from 1.1 to 3.0: where the bilinear view aliases
ALIASING_SHAPES = [((64, 128), (9, 16), 90.0), ((64, 128), (17, 31), 120.0), ((48, 96), (9, 16), 60.0), ((33, 66), (5, 7), 90.0)]


def stripes(H, W):
    """1-pixel vertical stripes, float64 [H, W, 1] of 0 / 1."""
    return np.broadcast_to((np.arange(W) % 2).astype(np.float64)[None, :, None], (H, W, 1)).copy()


def checker(H, W):
    """The 1-pixel checker, float64 [H, W, 1] of 0 / 1."""
    return ((np.arange(H)[:, None] + np.arange(W)[None, :]) % 2).astype(np.float64)[:, :, None]


def noise(seed, H, W):
    """White noise in [0, 1), float64 [H, W, 1]."""
    return np.random.default_rng(seed).random((H, W, 1))


def rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))
