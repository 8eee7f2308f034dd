"""numpy restatement of the reference's flow resize, cv2.resize(flow, (2 flow_h, flow_h), interpolation=cv2.INTER_CUBIC) *
(flow_h / W) (temporal_model/train_temporal.py:110-113), written from OpenCV's generic float path:

  * inv_scale = (double)dst / src, scale = 1.0 / inv_scale;
  * f = (float)((d + 0.5) * scale - 0.5), s = floor(f), f -= s;
  * coefficients in float, A = -0.75f:
      c0 = ((A (f+1) - 5A)(f+1) + 8A)(f+1) - 4A,   c1 = ((A+2) f - (A+3)) f^2 + 1,
      c2 = ((A+2)(1-f) - (A+3))(1-f)^2 + 1,       c3 = 1 - c0 - c1 - c2;
  * taps s-1 .. s+2, clamped to [0, n-1] on both axes (replicate);
  * horizontal pass first, then vertical;
  * equal sizes: cv2 copies the input.

The tables are built in float32 exactly as the spec says; the resize itself runs in float64 here (the library accumulates in
float32).  cv2 is not a test dependency, so this pins the restatement, not cv2 itself; an IPP build of OpenCV may differ in the
last bits.
"""
import numpy as np


def cubic_tables(n_in, n_out):
    """One axis: s int32 [n_out] (the tap s is the second of four) and the float32 coefficients [n_out, 4]."""
    inv_scale = float(n_out) / n_in
    scale = 1.0 / inv_scale
    A = np.float32(-0.75)
    one = np.float32(1.0)
    ofs = np.empty(n_out, np.int32)
    coef = np.empty((n_out, 4), np.float32)
    for d in range(n_out):
        f = np.float32((d + 0.5) * scale - 0.5)
        s = int(np.floor(f))
        f = np.float32(f - np.float32(s))
        x1 = np.float32(f + one)
        c0 = np.float32(np.float32(np.float32(np.float32(np.float32(A * x1) - np.float32(5) * A) * x1) + np.float32(8) * A) * x1
                        - np.float32(4) * A)
        c1 = np.float32(np.float32(np.float32(np.float32(np.float32(A + np.float32(2)) * f) - np.float32(A + np.float32(3))) * f)
                        * f + one)
        g = np.float32(one - f)
        c2 = np.float32(np.float32(np.float32(np.float32(np.float32(A + np.float32(2)) * g) - np.float32(A + np.float32(3))) * g)
                        * g + one)
        c3 = np.float32(np.float32(np.float32(one - c0) - c1) - c2)
        ofs[d] = s
        coef[d] = (c0, c1, c2, c3)
    return ofs, coef


def _axis(a, n_in, n_out, axis):
    """The pass along one axis of a float64 array."""
    if n_in == n_out:
        return a
    ofs, coef = cubic_tables(n_in, n_out)
    idx = np.clip(ofs[:, None] - 1 + np.arange(4)[None, :], 0, n_in - 1)          # [n_out, 4]
    taps = np.take(a, idx, axis=axis)                                                 # axis -> (n_out, 4)
    shape = [1] * taps.ndim
    shape[axis], shape[axis + 1] = n_out, 4
    return np.sum(taps * coef.astype(np.float64).reshape(shape), axis=axis + 1)


def resize(flow, h_out, w_out):
    """cv2.resize(INTER_CUBIC) of float flow [..., H, W, 2] to [..., h_out, w_out, 2] in float64 (no scale)."""
    a = np.asarray(flow, np.float64)
    h_in, w_in = a.shape[-3], a.shape[-2]
    if (h_in, w_in) == (h_out, w_out):
        return a.copy()
    a = _axis(a, w_in, w_out, a.ndim - 2)             # horizontal first
    return _axis(a, h_in, h_out, a.ndim - 3)


def resize_flow(flow, flow_h):
    """The reference's :110-113: resize to (flow_h, 2 flow_h), times flow_h / W of the original flow (float64)."""
    return resize(flow, flow_h, 2 * flow_h) * (flow_h / float(np.shape(flow)[-2]))
