"""Child process of tests/test_clstm_window_multi.py: cp360_clstm_window_multi against one cp360_clstm_window call per group on a
small cell (32 input / 32 hidden channels) in the Winograd domain.  The library runs so small a cell on the direct kernels unless
CP360_WINO=1 is set, and reads that variable once per process - hence this process, started with it.  Prints one JSON line:
{case: {'wino': both clip counts are the Winograd plan, 'h_out' / 'h_all' / 'minmax': equal bit for bit, 'finite': ...}}."""
import ctypes as C
import json

import numpy as np
import torch

from cp_360_weakly_supervised_saliency_amd import _lib
from cp_360_weakly_supervised_saliency_amd.utils import hashrng

DEV = 'cuda'
CH, T, GROUPS = 32, 3, 2
CASES = [(4, 7), (1, 8)]            # (clips per group, face): 768 tiles = two tile blocks, odd face; 96 tiles in one padded block, even face


def make_cell(L, prec, face, seed=8100):
    """A context with the synthetic cell loaded (and its Winograd filters, when the library would use them)."""
    c4 = 4 * CH
    g = lambda k, shape, std: torch.from_numpy(hashrng.normal(seed + k, shape, 0, std)).to(DEV)
    std = (2.0 / (9 * c4)) ** 0.5
    ws = [g(1, (c4, 2 * CH, 3, 3), std), g(2, (c4,), 0.05), g(3, (c4, c4, 3, 3), std), g(4, (c4,), 0.05),
          g(5, (c4, c4, 3, 3), std), g(6, (c4,), 0.05)]
    h = C.c_void_p()
    _lib.check(L.cp360_create(torch.cuda.current_device(), C.byref(h)))
    p = _lib.ptr
    code = _lib.dtype_code(_lib.precision_dtype(prec))
    _lib.check(L.cp360_clstm_load(h, code, *[p(t) for t in ws], CH, CH, face, _lib.stream()))
    if any(L.cp360_clstm_wino_state(h, n, face) == 2 for n in (1, 2, 4, 8)):
        _lib.check(L.cp360_clstm_load_wino(h, p(ws[0]), p(ws[2]), p(ws[4]), _lib.stream()))
    torch.cuda.synchronize()
    return h


def cams_of(n, face, seed):
    """GROUPS separately allocated CAM buffers [n, T, 6 face^2, CH] with distinct ranges per clip."""
    P = 6 * face * face
    return [torch.from_numpy(hashrng.uniform(seed + g, (n, T, P, CH), -1.0 - g, 2.0 + g)).to(DEV) for g in range(GROUPS)]


def run_window(L, h, prec, cam, n, face):
    P, dt = 6 * face * face, _lib.precision_dtype(prec)
    f = lambda *s: torch.empty(s, dtype=torch.float32, device=DEV)
    xh = torch.empty((n * P, 2 * CH), dtype=dt, device=DEV)
    c0, c1, h_out, h_all, mm, scr = f(n * P, CH), f(n * P, CH), f(n * P, CH), f(T, n * P, CH), f(n, 2), f(n * 512)
    nb = L.cp360_clstm_window_workspace_bytes(h, n, T, face)
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    p = _lib.ptr
    _lib.check(L.cp360_clstm_window(h, p(cam), 0, n, T, face, p(xh), p(c0), p(c1), p(h_out), p(h_all), p(mm), p(scr), p(ws), nb,
                                    _lib.stream()))
    return h_out, h_all, mm


def run_multi(L, h, cams, n, face, with_all=True):
    P, G = 6 * face * face, len(cams)
    f = lambda *s: torch.empty(s, dtype=torch.float32, device=DEV)
    h_outs, h_alls, mm = [f(n * P, CH) for _ in range(G)], [f(T, n * P, CH) for _ in range(G)], f(G * n, 2)
    nb = L.cp360_clstm_window_multi_workspace_bytes(h, G, n, T, face)
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    arr = lambda ts: (C.c_void_p * G)(*[t.data_ptr() for t in ts])
    _lib.check(L.cp360_clstm_window_multi(h, arr(cams), 0, G, n, T, face, arr(h_outs), arr(h_alls) if with_all else None,
                                          _lib.ptr(mm), _lib.ptr(ws), nb, _lib.stream()))
    return h_outs, h_alls, mm


def main():
    L = _lib.lib()
    out = {}
    for prec in ('bf16', 'fp16'):
        for n, face in CASES:
            h = make_cell(L, prec, face)
            try:
                wino = L.cp360_clstm_wino_state(h, n, face) == 1 and L.cp360_clstm_wino_state(h, GROUPS * n, face) == 1
                cams = cams_of(n, face, 8200 + 10 * face)
                singles = [run_window(L, h, prec, cam, n, face) for cam in cams]
                h_outs, h_alls, mm = run_multi(L, h, cams, n, face)
                h_only, _, _ = run_multi(L, h, cams, n, face, with_all=False)
                torch.cuda.synchronize()
                eq = lambda a, b: bool(torch.equal(a, b))
                out['%s-%dx%d' % (prec, n, face)] = {
                    'wino': bool(wino),
                    'h_out': all(eq(h_outs[g], singles[g][0]) and eq(h_only[g], singles[g][0]) for g in range(GROUPS)),
                    'h_all': all(eq(h_alls[g], singles[g][1]) for g in range(GROUPS)),
                    'minmax': all(eq(mm[g * n:(g + 1) * n], singles[g][2]) for g in range(GROUPS)),
                    'finite': bool(all(np.isfinite(s[1].cpu().numpy()).all() for s in singles)),
                    # the two groups differ: a multi call that ran group 0 twice would not pass
                    'distinct': not eq(singles[0][0], singles[1][0]),
                }
            finally:
                L.cp360_destroy(h)
    print('MULTI_RESULT ' + json.dumps(out))


if __name__ == '__main__':
    main()
