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

``loss_terms`` at the end is the float64 reference of the flow loss for the GPU tests: the torch lines of ``flow_losses`` for
already-scaled flow of any [H, W] (tests/test_flow_cpu.py pins it to ``flow_losses`` where W = 2 H).
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


def loss_terms(maps, flow_scaled, mm_th):
    """The three sum-MSE terms of ``flow_losses`` (train_temporal.py:115-167 of the reference) for ALREADY SCALED flow of any
    size: maps torch [B, L + 1, mh, mw], flow_scaled torch [B, L, H, W, 2], both of one floating dtype (float64 for a reference).
    The same torch lines as ``flow_losses`` (bilinear ``F.interpolate`` and ``grid_sample``, align_corners False, zero padding;
    the mesh on the (size - 1) grid, built in float32 as ``generate_meshgrid`` does); no W = 2 H restriction, no rescaling.
    Returns (loss_sm, loss_temp, loss_mask), differentiable with respect to maps (the next map of each pair only)."""
    import torch
    import torch.nn.functional as F
    B, n, _, _ = maps.shape
    L, H, W = flow_scaled.shape[1], flow_scaled.shape[2], flow_scaled.shape[3]
    assert n == L + 1 and flow_scaled.shape[0] == B
    y = torch.arange(0, H).unsqueeze(1).repeat(1, W) / (H - 1) * 2 - 1
    x = torch.arange(0, W).unsqueeze(0).repeat(H, 1) / (W - 1) * 2 - 1
    mesh = torch.stack([x, y], -1).float().to(maps.dtype)[None]                       # [1, H, W, 2]
    terms = [0, 0, 0]
    for b in range(B):
        for l in range(L):
            fl = flow_scaled[b, l]
            static = torch.sqrt(fl[..., 0] ** 2 + fl[..., 1] ** 2) < mm_th
            cur = F.interpolate(maps[b, l][None, None], size=(H, W), mode='bilinear', align_corners=False)
            nxt = F.interpolate(maps[b, l + 1][None, None], size=(H, W), mode='bilinear', align_corners=False)
            grid = torch.stack([fl[..., 0] / W * 2, fl[..., 1] / H * 2], -1)[None] + mesh
            warp = F.grid_sample(cur, grid, mode='bilinear', padding_mode='zeros', align_corners=False).detach()
            masked = nxt.detach().clone()
            masked[:, :, static] = 0
            for k, target in enumerate((warp, cur.detach(), masked)):
                terms[k] = terms[k] + ((nxt - target) ** 2).sum()
    return tuple(terms)
