"""Fine-tuning the ConvLSTM on ground truth: the loss is the metric ``utils.eval_sphere.SphereEval`` reports - K14's KL, CC and
NSS, weighted by solid angle, on K14's evaluation grid, through K14's resampler - with its gradient, in libcp360.so
(csrc/suploss.hip, DESIGN.md "K18").  The ground truth comes from ``utils.fixations.FixationMaps`` (density, mask) or
``utils.headtrack.HeadMaps``; the window's maps from ``model.clstm_train.window_maps``; the step from ``torch.optim.Adam`` or
``train_temporal.FusedAdam``.

    loss = cfg.l_kl * kl - cfg.l_cc * cc - cfg.l_nss * nss        (KL falls, CC and NSS rise)

Each of kl, cc, nss is the mean over the maps on which K14 defines the term (a map with a non-finite value, no variance, no mass
above its minimum, or no / only fixated pixels drops out of that term's mean and receives no gradient from it).  The KL's
``eps`` is ``cfg.kl_eps`` (default: the metric's 2^-52).  At 2^-52 a grid pixel whose value ties the map's minimum without
being its first occurrence has P = 0 and the slope -Q / eps, about 1e10 times a typical one: that is the true one-sided slope of
this KL, and a larger ``kl_eps`` (1e-7 .. 1e-3) is what tames it for training.  ``supervised_losses_torch`` composes the same
definition from torch operations: the CPU path, and the reference the device path is tested against.  The flow loss
(``train_temporal.device_flow_losses``) and this one are both autograd functions of the window's maps: add them to train on
both.
"""
import numpy as np
import torch

from .. import ops
from ..model.clstm_train import window_maps
from .train_temporal import _stack, normalize_batch

KL_EPS = 2.0 ** -52


class DeviceSupLoss(torch.autograd.Function):
    """(kl, cc, nss, valid) = DeviceSupLoss.apply(maps, G, fix, weights, kl_eps): maps f32 [N, mh, mw], G f32 [N, h, w], fix u8 /
    bool [N, h, w] or None, weights int32 [h] (``ops.sphere_eval_weights``) -> three f64 [N] (NaN where K14 defines none) and
    valid u8 [N, 3], in HIP on the launch stream without a synchronisation.  The gradient reaches maps only; an invalid term
    sends exactly 0 whatever gradient arrives for it."""

    @staticmethod
    def forward(ctx, maps, G, fix, weights, kl_eps):
        maps = maps.detach().float().contiguous()
        G = G.detach().float().contiguous()
        fix = None if fix is None else fix.detach().contiguous()
        terms, valid, stats = ops.sup_loss_forward(maps, G, weights, fix, kl_eps)
        ctx.save_for_backward(maps, G, weights, stats, valid)
        ctx.fix, ctx.kl_eps = fix, kl_eps
        ctx.mark_non_differentiable(valid)
        return terms[:, 0], terms[:, 1], terms[:, 2], valid

    @staticmethod
    def backward(ctx, g_kl, g_cc, g_nss, _g_valid):
        maps, G, weights, stats, valid = ctx.saved_tensors
        z = lambda g: torch.zeros(maps.shape[0], dtype=torch.float64, device=maps.device) if g is None else g.double()
        gterms = torch.stack([z(g_kl), z(g_cc), z(g_nss)], 1).contiguous()
        dmaps = ops.sup_loss_backward(maps, G, weights, stats, valid, gterms, ctx.fix, ctx.kl_eps)
        return dmaps, None, None, None, None


class DeviceSphereResample(torch.autograd.Function):
    """S = DeviceSphereResample.apply(maps, hw): maps f32 [N, mh, mw] -> f32 [N, h, w], the conservative remap on the sphere (K25,
    ``ops.sphere_resample``) with its adjoint (``ops.sphere_resample_adjoint``) as the gradient, both in HIP on the launch stream.
    In front of ``DeviceSupLoss`` it brings maps finer than the loss grid down; the loss then sees grid-sized maps and its own
    resampler copies."""

    @staticmethod
    def forward(ctx, maps, hw):
        maps = maps.detach().float().contiguous()
        ctx.src_hw = tuple(int(v) for v in maps.shape[1:])
        return ops.sphere_resample(maps, hw)

    @staticmethod
    def backward(ctx, g):
        return ops.sphere_resample_adjoint(g.float().contiguous(), ctx.src_hw), None


def _flatten(maps, gt, fixations):
    if maps.dim() != 4 or gt.dim() != 4 or tuple(gt.shape[:2]) != tuple(maps.shape[:2]):
        raise ValueError("maps must be [B, L, mh, mw] and gt [B, L, h, w], got %s and %s" % (tuple(maps.shape), tuple(gt.shape)))
    if fixations is not None and tuple(fixations.shape) != tuple(gt.shape):
        raise ValueError("fixations must have gt's shape %s, got %s" % (tuple(gt.shape), tuple(fixations.shape)))
    n = maps.shape[0] * maps.shape[1]
    return (maps.reshape(n, *maps.shape[2:]), gt.reshape(n, *gt.shape[2:]),
            None if fixations is None else fixations.reshape(n, *gt.shape[2:]))


def _valid_means(terms, valid):
    """terms: three [N], valid bool [N, 3] -> (three scalars, counts int64 [3]): each the mean over its valid maps, 0 (with a zero
    gradient) where there is none."""
    counts = valid.sum(dim=0, dtype=torch.int64)
    out = []
    for t in range(3):
        kept = torch.where(valid[:, t], terms[t], torch.zeros_like(terms[t]))
        out.append(kept.sum() / counts[t].clamp(min=1).to(kept.dtype))
    return out[0], out[1], out[2], counts


def supervised_losses(maps, gt, fixations=None, weights='solid_angle', kl_eps=KL_EPS, resample='bilinear'):
    """maps f32 [B, L, mh, mw] (the window's maps, on the GPU), gt f32 [B, L, h, w] on the loss grid, fixations u8 / bool
    [B, L, h, w] or None (K14's derived mask) -> (kl, cc, nss, counts): f64 scalars, differentiable with respect to maps, each
    the mean over that term's valid maps; counts int64 [3] = how many those are.  No synchronisation.  resample='conservative'
    brings the maps to the loss grid by ``DeviceSphereResample`` first (maps finer than the grid keep their mass)."""
    ops.check_resampler(resample)
    m, g, fx = _flatten(maps, gt, fixations)
    if resample == 'conservative':
        m = DeviceSphereResample.apply(m, tuple(g.shape[1:]))
    a = ops.sphere_eval_weights(g.shape[1], weights, m.device)
    kl, cc, nss, valid = DeviceSupLoss.apply(m, g, fx, a, float(kl_eps))
    return _valid_means((kl, cc, nss), valid != 0)


# ----------------------------------------------------------------------------- the same definition composed from torch
def _taps(n_dst, n_src, wrap):
    """The bilinear taps of csrc/sphere.h along one axis -> (i0, i1 int64 [n_dst], t float32 [n_dst]) as numpy arrays: the
    position and its fraction in float32 as the kernel computes them."""
    f32 = np.float32
    s = ((2.0 * np.arange(n_dst, dtype=np.float64) + 1.0) * n_src / (2.0 * n_dst) - 0.5).astype(f32)
    s = np.where(np.abs(s) <= f32(n_src), s, f32(0)) if wrap else np.minimum(np.maximum(s, f32(0)), f32(n_src - 1))
    i0f = np.floor(s)
    t = (s - i0f).astype(f32)
    if wrap:
        i0 = np.mod(i0f.astype(np.int64), n_src)
        return i0, np.where(i0 + 1 == n_src, 0, i0 + 1), t
    i0 = i0f.astype(np.int64)
    return i0, np.minimum(i0 + 1, n_src - 1), t


def resample_torch(maps, hw):
    """maps [N, mh, mw] -> [N, h, w] in maps' dtype: cp360_seval_resample's terms in its order (columns wrap, rows clamp; a map of
    the grid's size is returned as it is), differentiable."""
    h, w = hw
    if tuple(maps.shape[1:]) == (h, w):
        return maps
    dev = maps.device
    y0, y1, ty = _taps(h, maps.shape[1], False)
    x0, x1, tx = _taps(w, maps.shape[2], True)
    y0, y1, x0, x1 = (torch.from_numpy(v).to(dev) for v in (y0, y1, x0, x1))
    tx = torch.from_numpy(tx).to(dev, maps.dtype)[None, None, :]
    ty = torch.from_numpy(ty).to(dev, maps.dtype)[None, :, None]
    r0, r1 = maps[:, y0], maps[:, y1]
    v00, v01, v10, v11 = r0[:, :, x0], r0[:, :, x1], r1[:, :, x0], r1[:, :, x1]
    top = v00 + tx * (v01 - v00)
    bot = v10 + tx * (v11 - v10)
    return top + ty * (bot - top)


def _conservative_matrix(n_src, n_dst, axis):
    """The dense float32 [n_dst, n_src] matrix of one axis of the conservative remap, from the library's host tables."""
    start, count, weights = ops.sphere_resample_tables_host(n_src, n_dst, axis)
    M = np.zeros((n_dst, n_src), np.float32)
    for d in range(n_dst):
        for k in range(int(count[d])):
            i = int(start[d]) + k
            M[d, i % n_src if axis == 1 else min(i, n_src - 1)] += weights[d, k]
    return M


def resample_conservative_torch(maps, hw):
    """maps [N, mh, mw] -> [N, h, w] in maps' dtype: ``ops.sphere_resample``'s definition as two dense matrix
    products, Wy @ maps @ Wx^T with the library's host tables; differentiable.  The order of its sums is the matrix product's, not
    the kernel's: equal to the kernel within rounding, not bit for bit."""
    h, w = (int(v) for v in hw)
    Wy = torch.from_numpy(_conservative_matrix(int(maps.shape[1]), h, 0)).to(maps.device, maps.dtype)
    Wx = torch.from_numpy(_conservative_matrix(int(maps.shape[2]), w, 1)).to(maps.device, maps.dtype)
    return torch.matmul(torch.matmul(Wy, maps), Wx.t())


def _sum(x):
    return x.sum(dim=(1, 2))


def map_terms_torch(S, G, M, a, kl_eps):
    """S, G [N, h, w], M bool [N, h, w], a [h, 1] in S's dtype -> (kl, cc, nss) [N] each: DESIGN.md 7f's definitions."""
    A = a.sum() * S.shape[2]
    b = lambda v: v[:, None, None]
    s, g = S - b(_sum(a * S) / A), G - b(_sum(a * G) / A)
    Vs, Vg = _sum(a * s * s), _sum(a * g * g)
    cc = _sum(a * s * g) / torch.sqrt(Vs * Vg)
    n = M.sum(dim=(1, 2))
    nss = _sum(torch.where(M, s / b(torch.sqrt(Vs / A)), torch.zeros_like(s))) / n.to(S.dtype)
    nss = torch.where(n == S.shape[1] * S.shape[2], torch.full_like(nss, float('nan')), nss)
    # P is 0 at the minimum whatever S holds: written as that constant, so that autograd does not send k_mm (of the order
    # Q_mm / eps) down two paths that cancel; the value is the same bits
    flat = S.detach().reshape(S.shape[0], -1)
    first = torch.zeros_like(flat, dtype=torch.bool).scatter_(1, flat.argmin(dim=1, keepdim=True), True).reshape(S.shape)
    p = torch.where(first, torch.zeros_like(S), a * (S - b(S.amin(dim=(1, 2)))))
    q = a * (G - b(G.amin(dim=(1, 2))))
    p, q = p / b(_sum(p)), q / b(_sum(q))
    kl = _sum(q * torch.log(kl_eps + q / (p + kl_eps)))
    return kl, cc, nss


def supervised_losses_torch(maps, gt, fixations=None, weights='solid_angle', kl_eps=KL_EPS, resample='bilinear'):
    """``supervised_losses`` composed from torch operations in maps' dtype, on maps' device: the CPU path and the reference for the
    device path.  A term's valid maps are found first (one synchronisation) and only they enter its mean, so that a NaN never
    enters the graph.  The minimum's gradient is torch's (ties share it), where the kernel gives it to the first occurrence."""
    ops.check_resampler(resample)
    m, g, fx = _flatten(maps, gt, fixations)
    g = g.to(m.dtype)
    h, w = g.shape[1:]
    a = ops.sphere_eval_weights(h, weights, 'cpu').clamp(0, 1024).to(m.device, m.dtype)[:, None]
    S = resample_conservative_torch(m, (h, w)) if resample == 'conservative' else resample_torch(m, (h, w))
    with torch.no_grad():
        if fx is None:                                                 # K14's rule, decided in float64 as the kernel decides it
            ad, gd = a.double(), g.double()
            A = ad.sum() * w
            mu = _sum(ad * gd) / A
            sigma = torch.sqrt(_sum(ad * (gd - mu[:, None, None]) ** 2) / A)
            M = gd > (mu + 2.0 * sigma)[:, None, None]
        else:
            M = fx != 0
        finite = torch.isfinite(S).all(dim=2).all(dim=1) & torch.isfinite(g).all(dim=2).all(dim=1)
        valid = torch.stack([torch.isfinite(t) & finite for t in map_terms_torch(S, g, M, a, kl_eps)], 1)
    counts = valid.sum(dim=0, dtype=torch.int64)
    out = []
    for t in range(3):
        idx = valid[:, t].nonzero().flatten()
        if idx.numel() == 0:
            out.append(torch.zeros((), dtype=m.dtype, device=m.device))
        else:
            out.append(map_terms_torch(S[idx], g[idx], M[idx], a, kl_eps)[t].mean())
    return out[0], out[1], out[2], counts


# ----------------------------------------------------------------------------- one iteration
def train_step_gt(cell, seq, gt, optimizer, cfg, fixations=None, map_steps=None):
    """One iteration on one batch against ground truth: seq = T tensors [B, 6, C, w, w] (or [B, T, 6, C, w, w]), gt f32
    [B, L, h, w] on the loss grid for the steps ``map_steps`` (default: all T), fixations u8 / bool of gt's shape or None.
    Normalises as ``train_step`` does, takes ``window_maps``, loss = cfg.l_kl * kl - cfg.l_cc * cc - cfg.l_nss * nss with
    ``cfg.kl_eps`` (default 2^-52) and ``cfg.loss_weights`` (default 'solid_angle'), then ``optimizer.zero_grad();
    loss.backward(); optimizer.step()``.  Returns (kl, cc, nss, counts), detached."""
    dev = cell.Conv1.weight.device
    seq = _stack(seq).to(dev, torch.float32)
    if seq.dim() != 6 or seq.shape[2] != 6:
        raise ValueError("seq must be T tensors [B, 6, C, w, w]")
    B, T, _, C, w, _ = seq.shape
    steps = tuple(range(T)) if map_steps is None else tuple(int(s) for s in map_steps)
    gt = gt.to(dev, torch.float32)
    if gt.dim() != 4 or gt.shape[0] != B or gt.shape[1] != len(steps):
        raise ValueError("gt must be [B = %d, L = %d, h, w], got %s" % (B, len(steps), tuple(gt.shape)))
    if fixations is not None:
        fixations = fixations.to(dev)
    frames = normalize_batch(seq).permute(0, 1, 2, 4, 5, 3).reshape(B, T, 6 * w * w, C).contiguous()
    maps = window_maps(cell, frames, steps)
    kl, cc, nss, counts = supervised_losses(maps, gt, fixations, getattr(cfg, 'loss_weights', 'solid_angle'),
                                            getattr(cfg, 'kl_eps', KL_EPS))
    loss = cfg.l_kl * kl - cfg.l_cc * cc - cfg.l_nss * nss
    optimizer.zero_grad()
    loss.backward()
    optimizer.step()
    return kl.detach(), cc.detach(), nss.detach(), counts
