"""Float64 restatement of the supervised loss (K18, csrc/suploss.hip; the specification is DESIGN.md "K18") on top of
tests/sphere_eval_restate.py: K14's KL, CC and NSS of the resampled map, their gradient with respect to the grid values S, and
the adjoint of the resampler.  Written independently of the kernels: numpy sums, matrices for the taps.  Not a test file.

    s = S - mu_S, g = G - mu_G, Vs = sum_a s^2, Vg = sum_a g^2, A = sum a, sigma = sqrt(Vs / A), n = n_fix
    dCC/dS_j  = a_j (g_j / sqrt(Vs Vg) - CC s_j / Vs)
    dNSS/dS_j = ([j in M] / n - a_j / A) / sigma - NSS a_j s_j / (A sigma^2)
    KL: r_i = Q_i / (P_i + eps), k_i = -Q_i r_i / ((P_i + eps)(eps + r_i)), mm = the lowest index with S_mm = min S,
        K1 = sum_{i != mm} k_i P_i, K2 = sum_{i != mm} k_i a_i
        dKL/dS_j = a_j (k_j - K1) / Z for j != mm,  dKL/dS_mm = ((A - a_mm) K1 - K2) / Z
    dm = Ry^T dS Rx, Ry [h, mh] and Rx [w, mw] the row and column factors of the sampler's taps (f32 fractions, taken to double)
"""
import numpy as np

from tests import sphere_eval_restate as rs

EPS = rs.EPS
TERMS = ('kl', 'cc', 'nss')


# ----------------------------------------------------------------------------- the resampler as two matrices
def taps(n_dst, n_src, wrap):
    """(i0, i1 int64 [n_dst], t float64 [n_dst]): sphere.h's taps along one axis, the fraction computed in float32."""
    f32 = np.float32
    s = ((2.0 * np.arange(n_dst, dtype=np.float64) + 1.0) * n_src / (2.0 * n_dst) - 0.5).astype(f32)
    if wrap:
        s = np.where(np.abs(s) <= f32(n_src), s, f32(0))
    else:
        s = np.minimum(np.maximum(s, f32(0)), f32(n_src - 1))
    i0f = np.floor(s)
    t = (s - i0f).astype(f32)
    if wrap:
        i0 = np.mod(i0f.astype(np.int64), n_src)
        i1 = np.where(i0 + 1 == n_src, 0, i0 + 1)
    else:
        i0 = i0f.astype(np.int64)
        i1 = np.minimum(i0 + 1, n_src - 1)
    return i0, i1, t.astype(np.float64)


def tap_matrix(n_dst, n_src, wrap):
    """float64 [n_dst, n_src]: row i holds 1 - t at i0 and t at i1 (both at the one index where a clamp makes them meet)."""
    R = np.zeros((n_dst, n_src), np.float64)
    if n_dst == n_src:
        return np.eye(n_dst)
    i0, i1, t = taps(n_dst, n_src, wrap)
    np.add.at(R, (np.arange(n_dst), i0), 1.0 - t)
    np.add.at(R, (np.arange(n_dst), i1), t)
    return R


def matrices(mh, mw, h, w):
    """(Ry [h, mh], Rx [w, mw]); a map of the grid's size is copied: identities."""
    if (mh, mw) == (h, w):
        return np.eye(h), np.eye(w)
    return tap_matrix(h, mh, False), tap_matrix(w, mw, True)


def resample64(m, h, w):
    """The resampler in exact-weights float64, m [mh, mw] -> [h, w]: what autograd differentiates."""
    Ry, Rx = matrices(m.shape[0], m.shape[1], h, w)
    return Ry @ np.asarray(m, np.float64) @ Rx.T


def adjoint(dS, mh, mw):
    """dS float64 [h, w] -> dm float64 [mh, mw]."""
    Ry, Rx = matrices(mh, mw, dS.shape[0], dS.shape[1])
    return Ry.T @ dS @ Rx


# ----------------------------------------------------------------------------- forward
def forward(S, G, a_rows, M=None, eps=EPS):
    """S, G [h, w] (any float type, taken to float64), a_rows [h], M bool [h, w] or None -> dict with 'terms' float64 [3] = (kl,
    cc, nss), 'valid' bool [3], and the scalars of the gradient."""
    S, G = np.asarray(S, np.float64), np.asarray(G, np.float64)
    h, w = S.shape
    a = np.repeat(np.asarray(a_rows, np.float64)[:, None], w, axis=1)
    nan = float('nan')
    with np.errstate(all='ignore'):
        M = rs.derive_mask(G, a_rows) if M is None else np.asarray(M) != 0
        n = int(M.sum())
        bad = not (np.all(np.isfinite(S)) and np.all(np.isfinite(G)))
        A = a.sum()
        mu_s, mu_g = (a * S).sum() / A, (a * G).sum() / A
        s, g = S - mu_s, G - mu_g
        Vs, Vg, Csg = (a * s * s).sum(), (a * g * g).sum(), (a * s * g).sum()
        sigma = np.sqrt(Vs / A)
        cc = nan if bad else float(Csg / np.sqrt(Vs * Vg))
        nss = nan if bad or n == h * w else float((s[M] / sigma).sum() / np.float64(n))
        min_s, min_g = S.min(), G.min()
        Z, Zg = (a * (S - min_s)).sum(), (a * (G - min_g)).sum()
        p, q = a * (S - min_s) / Z, a * (G - min_g) / Zg
        kl = nan if bad or not (Z > 0 and Zg > 0) else float((q * np.log(eps + q / (p + eps))).sum())
        mm = h * w if np.isnan(S).any() else int(np.argmin(S.reshape(-1)))          # the lowest index of the minimum
        r = q / (p + eps)
        k = -(q * r) / ((p + eps) * (eps + r))
        keep = np.ones(h * w, bool)
        keep[mm:mm + 1] = False
        K1 = (k * p).reshape(-1)[keep].sum()
        K2 = (k * a).reshape(-1)[keep].sum()
        valid = np.array([np.isfinite(kl) and np.isfinite(K1) and np.isfinite(K2) and mm < h * w,
                          np.isfinite(cc) and Vs > 0 and Vg > 0,
                          np.isfinite(nss) and Vs > 0 and n > 0], bool)
    return dict(terms=np.array([kl, cc, nss], np.float64), valid=valid, a=a, M=M, n=n, A=A, s=s, g=g, Vs=Vs, Vg=Vg, sigma=sigma,
                Z=Z, p=p, q=q, k=k, K1=K1, K2=K2, mm=mm, cc=cc, nss=nss)


def grad_terms(fw):
    """The three gradients with respect to S of a forward() result, float64 [3, h, w], whatever `valid` says."""
    a, s, g, Vs, Vg, A, sigma = fw['a'], fw['s'], fw['g'], fw['Vs'], fw['Vg'], fw['A'], fw['sigma']
    with np.errstate(all='ignore'):
        d_cc = a * (g / np.sqrt(Vs * Vg) - fw['cc'] * s / Vs)
        d_nss = (fw['M'] / np.float64(fw['n']) - a / A) / sigma - fw['nss'] * a * s / (A * sigma * sigma)
        d_kl = a * (fw['k'] - fw['K1']) / fw['Z']
        if fw['mm'] < a.size:
            y, x = divmod(fw['mm'], a.shape[1])
            d_kl[y, x] = ((A - a[y, x]) * fw['K1'] - fw['K2']) / fw['Z']
    return np.stack([d_kl, d_cc, d_nss])


def grad_S(fw, gterms):
    """dS float64 [h, w] = sum_t gterms_t valid_t dterm_t/dS; an invalid term, or a gterms entry of 0, adds nothing."""
    d = grad_terms(fw)
    out = np.zeros_like(fw['a'])
    for t in range(3):
        if fw['valid'][t] and gterms[t] != 0.0:
            out = out + np.float64(gterms[t]) * d[t]
    return out


def loss(maps, G, a_rows, fix=None, eps=EPS, exact=False):
    """maps f32 [N, mh, mw], G f32 [N, h, w] -> the forward() of every map on S = the float32 resampler's output (exact: on the
    float64 resampler's)."""
    N, h, w = G.shape
    S = [resample64(m, h, w) for m in maps] if exact else rs.resample(np.asarray(maps, np.float32), h, w)
    return [forward(S[n], G[n], a_rows, None if fix is None else fix[n], eps) for n in range(N)]


def backward(maps, G, a_rows, gterms, fix=None, eps=EPS, exact=False):
    """-> (terms float64 [N, 3], valid bool [N, 3], dmaps float64 [N, mh, mw], the forward() results)."""
    fws = loss(maps, G, a_rows, fix, eps, exact)
    mh, mw = maps.shape[1:]
    dm = np.stack([adjoint(grad_S(fw, gterms[n]), mh, mw) for n, fw in enumerate(fws)])
    return np.stack([fw['terms'] for fw in fws]), np.stack([fw['valid'] for fw in fws]), dm, fws


# ----------------------------------------------------------------------------- the same forward in torch float64, for autograd
def torch_terms(m, G, a_rows, M, hw, eps=EPS):
    """m a float64 torch tensor [mh, mw] (requires_grad), G float64 numpy [h, w], M bool numpy [h, w] -> (kl, cc, nss) as torch
    scalars: the restated forward through the float64 resampler, composed from differentiable operations."""
    import torch
    h, w = hw
    Ry, Rx = (torch.from_numpy(R) for R in matrices(m.shape[0], m.shape[1], h, w))
    S = Ry @ m @ Rx.T
    G = torch.from_numpy(np.asarray(G, np.float64))
    a = torch.from_numpy(np.repeat(np.asarray(a_rows, np.float64)[:, None], w, axis=1))
    Mt = torch.from_numpy(np.asarray(M, bool))
    A = a.sum()
    s, g = S - (a * S).sum() / A, G - (a * G).sum() / A
    Vs, Vg = (a * s * s).sum(), (a * g * g).sum()
    cc = (a * s * g).sum() / torch.sqrt(Vs * Vg)
    nss = (s[Mt] / torch.sqrt(Vs / A)).sum() / float(Mt.sum())
    # P_mm is 0 whatever S holds: written as the constant it is, so that autograd does not send k_mm (of the order Q_mm / eps) down
    # two paths that cancel - the forward value is bit for bit the same
    first = torch.zeros(h * w, dtype=torch.bool)
    first[int(torch.argmin(S.detach().reshape(-1)))] = True
    p, q = torch.where(first.reshape(h, w), torch.zeros_like(S), a * (S - S.min())), a * (G - G.min())
    p, q = p / p.sum(), q / q.sum()
    kl = (q * torch.log(eps + q / (p + eps))).sum()
    return kl, cc, nss


# ----------------------------------------------------------------------------- inputs the CPU and GPU tests share
def case(seed, N, mh, mw, h, w):
    """(maps f32 [N, mh, mw], G f32 [N, h, w], fix bool [N, h, w]): sphere_eval_restate.video's blobs on noise; the explicit
    mask is the 5 % highest pixels of each G."""
    maps, G = rs.video(seed, N, mh, mw, h, w)
    fix = np.stack([g >= np.quantile(g, 0.95) for g in G])
    return maps, G, fix


def unique_min(m, hw, at=None, low=-4.0):
    """A copy of the float32 map m [mh, mw] (values in 0 .. 2) whose minimum is the one pixel `at`, lowered to `low`; the default
    is the heavier tap of the h x w grid's central pixel, so that a grid coarser than the map sees it with a weight of at least a
    quarter: the grid's minimum lies there, well below every other pixel."""
    m = np.array(m, np.float32)
    if at is None:
        (y0, y1, ty), (x0, x1, tx) = taps(hw[0], m.shape[0], False), taps(hw[1], m.shape[1], True)
        cy, cx = hw[0] // 2, hw[1] // 2
        at = (y0[cy] if ty[cy] < 0.5 else y1[cy], x0[cx] if tx[cx] < 0.5 else x1[cx])
    y, x = at
    m[y, x] = low
    return m
