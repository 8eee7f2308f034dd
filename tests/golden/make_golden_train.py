#!/usr/bin/env python3
"""Generate tests/golden/clstm_train.npz by RUNNING THE REFERENCE's own ``train()`` (temporal_model/train_temporal.py:33-193).

Runs only in the build container (needs /root/reference, read-only); nothing of the reference's source is written to the
repository - the fixture holds the hash-RNG seeds of the inputs and the reference's outputs.  Shims, all in memory, on top
of those of make_golden.py:
  * the source of train_temporal.py is exec'd with ``.cuda(async=True)`` deleted and ``.cuda()`` -> ``.clone()``;
  * cv2 is a stub whose ``resize`` is the identity when the size already matches (anything else raises);
  * stub modules for ruamel_yaml, torchvision.transforms, data.dataset and utils.utils (imported, unused by train()).

Run: ConvLSTMCell(8, 8) with synthetic weights (synth.clstm_state), w = 7, B = 2, seq_len 5, flow_h 28, Adam, two
iterations on a list loader.  Recorded: the three loss terms per iteration, every parameter's gradient in iteration 1,
every parameter after iteration 2, and the saliency maps of iteration 1 (the input of the loss).

    python tests/golden/make_golden_train.py
"""
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = '/root/reference'
sys.path.insert(0, REPO)

from cp_360_weakly_supervised_saliency_amd.utils import hashrng, synth  # noqa: E402

B, T, CH, W, FLOW_H, ITERS = 2, 5, 8, 7, 28, 2
SEQ_SEED, FLOW_SEED, STATE_SEED = 7100, 7200, 71
CFG = dict(seq_len=T, flow_h=FLOW_H, l_s=0.7, l_t=1.0, l_m=0.01, mm_th=0.15, use_gpu=True, summary_freq=1,
           save_freq=1000, lr=1e-3)


def batch(it):
    """Loader item ``it``: seq = T tensors [B, 6, CH, W, W], flow = T tensors [B, FLOW_H, 2 FLOW_H, 2] (numpy)."""
    seq = [hashrng.uniform(SEQ_SEED + 10 * it + t, (B, 6, CH, W, W), 0.0, 4.0) for t in range(T)]
    flow = [hashrng.normal(FLOW_SEED + 10 * it + t, (B, FLOW_H, 2 * FLOW_H, 2), 0.0, 0.4) for t in range(T)]
    return seq, flow


def main():
    from make_golden import import_reference
    R = import_reference()
    torch = R['torch']
    cv2 = sys.modules['cv2']
    cv2.INTER_CUBIC = 2

    def resize(src, dsize, interpolation=None):
        if tuple(src.shape[:2]) != (dsize[1], dsize[0]):
            raise ValueError("cv2 stub: only the identity resize is available")
        return np.array(src, copy=True)
    cv2.resize = resize
    for name in ('ruamel_yaml', 'torchvision.transforms', 'data', 'data.dataset', 'utils.utils'):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules['torchvision'].transforms = sys.modules['torchvision.transforms']
    sys.modules['data.dataset'].Sal360Dataset = None
    sys.modules['utils.utils'].cam_visual = None
    sys.modules['utils.cube_to_equi'] = R['c2e']
    src = open(os.path.join(REF, 'temporal_model/train_temporal.py')).read()
    src = src.replace('.cuda(async=True)', '').replace('.cuda()', '.clone()')
    mod = types.ModuleType('ref_train_temporal')
    mod.__file__ = os.path.join(REF, 'temporal_model/train_temporal.py')
    exec(compile(src, mod.__file__, 'exec'), mod.__dict__)

    # record to_equi_nn outputs (-> the maps) and every criterion call (-> the loss terms, summed as train() sums them)
    maps, calls = [], []
    c2e_cls = mod.Cube2Equi

    class RecC2E(c2e_cls):
        def to_equi_nn(self, x):
            out = c2e_cls.to_equi_nn(self, x)
            maps.append(torch.max(out, 1)[0].detach().numpy()[0])
            return out
    mod.Cube2Equi = RecC2E
    mse = torch.nn.MSELoss(reduction='sum')

    def criterion(a, b):
        v = mse(a, b)
        calls.append(v.detach().clone())
        return v

    sd = synth.clstm_state(seed=STATE_SEED, input_size=CH, hidden_size=CH)
    cell = R['clstm'].ConvLSTMCell(CH, CH)
    cell.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    R['cpu_pads'](cell)
    opt = torch.optim.Adam(cell.parameters(), lr=CFG['lr'])
    grads = {}
    step = opt.step

    def rec_step(*a, **k):
        if not grads:
            grads.update({n: p.grad.detach().numpy().copy() for n, p in cell.named_parameters()})
        return step(*a, **k)
    opt.step = rec_step
    loader = []
    for it in range(ITERS):
        seq, flow = batch(it)
        loader.append(([torch.from_numpy(s) for s in seq], [torch.from_numpy(f) for f in flow], 'cat', '000000.npy'))
    cfg = types.SimpleNamespace(**CFG)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        mod.train(loader, cell, criterion, opt, 0, '/nonexistent', 0, cfg, tmp_loss_len=3)

    per = 3 * B * 3                                          # criterion calls per iteration (B clips x 3 pairs x 3 terms)
    assert len(calls) == ITERS * per, len(calls)
    out = dict(cfg_keys=np.array(sorted(CFG)), cfg_vals=np.array([float(CFG[k]) for k in sorted(CFG)]),
               seeds=np.array([SEQ_SEED, FLOW_SEED, STATE_SEED, B, T, CH, W, FLOW_H, ITERS]))
    losses = np.zeros((ITERS, 3), dtype=np.float32)
    for it in range(ITERS):
        c = calls[it * per:(it + 1) * per]
        for k in range(3):
            acc = c[k].clone()
            for j in range(1, per // 3):
                acc += c[3 * j + k]
            losses[it, k] = acc.item()
    out['losses'] = losses
    nmap = 4 * B                                             # steps 1..4 x B clips per iteration, step-major
    m1 = np.stack(maps[:nmap]).reshape(4, B, 2 * W, 4 * W).transpose(1, 0, 2, 3)
    out['maps_it0'] = np.ascontiguousarray(m1, dtype=np.float32)
    for n, g in grads.items():
        out['grad_' + n] = g.astype(np.float32)
    for n, p in cell.state_dict().items():
        out['after_' + n] = p.numpy().astype(np.float32)
    np.savez_compressed(os.path.join(HERE, 'clstm_train.npz'), **out)
    print('clstm_train.npz written: losses', losses.tolist())


if __name__ == '__main__':
    sys.path.insert(0, HERE)
    main()
