"""Stage-planner equivalence: what the stage contexts of csrc/ctx.hip plan - cp360_resnet_plan_describe (return value and full
text), cp360_resnet_workspace_bytes, the status codes of refused calls, cp360_clstm_wino_state, cp360_clstm_workspace_bytes and
cp360_clstm_window_workspace_bytes - against tests/golden/stage_plans.json, recorded from the library BEFORE the planner became
one step list (plan_resnet / plan_clstm) that the launcher, the sizer and the describer share.  Every entry must be equal.

A context needs a device to be created and loaded, so the comparison is a GPU test; nothing but the weight packing is launched.

Recording (on a GPU, against a build of the commit to compare with):
    CP360_LIB=<that build>/libcp360.so python -m tests.test_stage_plan --record <its commit hash>
"""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

from cp_360_weakly_supervised_saliency_amd import _lib
from cp_360_weakly_supervised_saliency_amd.utils import hashrng, synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'stage_plans.json')
DEV = 'cuda'
PRECISIONS = (('fp32', _lib.F32), ('bf16', _lib.BF16), ('fp16', _lib.F16))
STATIC_SHAPES = ((6, 224), (12, 224), (24, 224), (96, 224), (384, 224), (6, 32), (6, 64), (6, 96), (6, 256), (384, 256),
                 (6, 512), (96, 512))
CHEAP_FACES, CHEAP_CLIPS = (4, 7, 8, 9, 16), (1, 2, 4)
REAL_SHAPES = ((7, 1), (7, 4), (8, 2))                       # (face, clips) of the 1000 / 1000 cell, loaded once (at face 7)

# every branch of the static-stage planner leaves one of these in a recorded text (checked when recording and on the fixture)
NOTE_LINES = (
    'stem: FUSED stem', 'stem: resident-patch stem kernel', 'stem: generic convolution',
    'layer1: ONE fused launch per Bottleneck', 'layer1: conv1 of block 0, then ONE fused launch', 'layer1: GENERIC path',
    'layer2.0: ONE fused launch after its conv1', 'layer2.0: generic path', 'layer3.0: generic path',
    'layer2.1-3: conv1 + ONE fused tail launch', 'layer2.1-3: GENERIC path',
    'layer3.1-5: conv1 + ONE fused tail launch', 'layer3.1-5: GENERIC path',
    'layer4: one launch per convolution', 'CAM: 1x1 convolution with the shifted fc.weight')


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _resnet_arrays():
    """(the 53 cp360_conv_bn of synth.resnet50_state(seed=1), fc.weight, fc shift, the device tensors that back them)"""
    sd = synth.resnet50_state(seed=1)
    dev = {k: _dev(v) for k, v in sd.items() if 'num_batches' not in k}
    names = [('conv1', 'bn1')]
    for layer, nb in (('layer1', 3), ('layer2', 4), ('layer3', 6), ('layer4', 3)):
        for b in range(nb):
            names += [('%s.%d.conv%d' % (layer, b, i), '%s.%d.bn%d' % (layer, b, i)) for i in (1, 2, 3)]
            if b == 0:
                names.append(('%s.0.downsample.0' % layer, '%s.0.downsample.1' % layer))
    pairs = [_lib.ConvBn(*[dev[k].data_ptr() for k in (c + '.weight', bn + '.weight', bn + '.bias', bn + '.running_mean',
                                                         bn + '.running_var')]) for c, bn in names]
    fc = dev['fc.weight']
    mn = float(fc.min())
    return (_lib.ConvBn * 53)(*pairs), fc, (mn if mn < 0 else 0.0), dev


class _Ctx:
    def __init__(self, L):
        self.L, self.h = L, C.c_void_p()
        _lib.check(L.cp360_create(0, C.byref(self.h)))

    def __enter__(self):
        return self.h

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        self.L.cp360_destroy(self.h)


def _describe(L, h, n_img, cd, cap=1 << 15):
    buf = C.create_string_buffer(cap)
    rc = L.cp360_resnet_plan_describe(h, n_img, cd, buf, cap)
    return rc, buf.value.decode()


def _static(L):
    """{precision: {'<n_img>x<cube>': [describe rc, text, workspace bytes]}} and {precision: {bad call: status}}"""
    arr, fc, shift, keep = _resnet_arrays()
    dummy = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    base = dummy.data_ptr() + (-dummy.data_ptr()) % 256           # a 256-byte aligned address with 1024 bytes behind it
    p = C.c_void_p
    plans, refusals = {}, {}
    for prec, code in PRECISIONS:
        with _Ctx(L) as h:
            r = refusals[prec] = {}
            r['describe before load'] = _describe(L, h, 6, 224)[0]
            r['workspace before load'] = L.cp360_resnet_workspace_bytes(h, 6, 224)
            r['forward before load'] = L.cp360_resnet_forward(h, p(base), 6, 224, p(base), None, p(base), 1024, None)
            _lib.check(L.cp360_resnet_load(h, code, arr, 53, p(fc.data_ptr()), 1000, shift, 1e-5, None))
            plans[prec] = {}
            for n_img, cd in STATIC_SHAPES:
                rc, text = _describe(L, h, n_img, cd)
                plans[prec]['%dx%d' % (n_img, cd)] = [rc, text, L.cp360_resnet_workspace_bytes(h, n_img, cd)]
            # the refused calls: every check returns before anything is launched
            for n_img, cd in ((5, 224), (0, 224), (6, 48), (6, 0)):
                r['describe %dx%d' % (n_img, cd)] = _describe(L, h, n_img, cd)[0]
                r['workspace %dx%d' % (n_img, cd)] = L.cp360_resnet_workspace_bytes(h, n_img, cd)
                r['forward %dx%d' % (n_img, cd)] = L.cp360_resnet_forward(h, p(base), n_img, cd, p(base), None, p(base), 1024, None)
            r['describe into 16 bytes'] = list(_describe(L, h, 6, 224, cap=16))
            r['describe into no buffer'] = L.cp360_resnet_plan_describe(h, 6, 224, None, 0)
            r['forward, 1024-byte workspace'] = L.cp360_resnet_forward(h, p(base), 6, 224, p(base), None, p(base), 1024, None)
            r['forward, misaligned workspace'] = L.cp360_resnet_forward(h, p(base), 6, 224, p(base), None, p(base + 1), 1024, None)
            r['forward, null faces'] = L.cp360_resnet_forward(h, None, 6, 224, p(base), None, p(base), 1024, None)
            r['forward, null cam'] = L.cp360_resnet_forward(h, p(base), 6, 224, None, None, p(base), 1024, None)
    del keep
    return plans, refusals


def _cell_answers(L, h, clips, face):
    return [L.cp360_clstm_wino_state(h, clips, face), L.cp360_clstm_workspace_bytes(h, clips, face),
            L.cp360_clstm_window_workspace_bytes(h, clips, 1, face), L.cp360_clstm_window_workspace_bytes(h, clips, 5, face)]


def _clstm(L):
    """{'<cell> <precision> face <f> clips <n>': [wino state, step workspace, window workspace at T = 1, at T = 5]}; the first shape
    that answers state 2 gets its Winograd filters loaded and is asked again ('... + load_wino')."""
    out = {}
    reloaded = [False]

    def cell(name, code, prec, ws, cin, ch, load_face, shapes):
        with _Ctx(L) as h:
            _lib.check(L.cp360_clstm_load(h, code, *[C.c_void_p(t.data_ptr()) for t in ws], cin, ch, load_face, None))
            for face, clips in shapes:
                key = '%s %s face %d clips %d' % (name, prec, face, clips)
                out[key] = _cell_answers(L, h, clips, face)
                if out[key][0] == 2 and not reloaded[0]:
                    reloaded[0] = True
                    _lib.check(L.cp360_clstm_load_wino(h, *[C.c_void_p(ws[i].data_ptr()) for i in (0, 2, 4)], None))
                    out[key + ' + load_wino'] = _cell_answers(L, h, clips, face)
                    # (the later shapes of this load are asked with the filters resident: state 1 where it was 2)

    def weights(seed, cin, ch):
        c4 = 4 * ch
        return [_dev(hashrng.normal(seed + i, s, 0.0, 0.05)) for i, s in
                enumerate(((c4, cin + ch, 3, 3), (c4,), (c4, c4, 3, 3), (c4,), (c4, c4, 3, 3), (c4,)))]
    cheap = weights(9100, 64, 64)
    for prec, code in PRECISIONS[:2]:
        for face in CHEAP_FACES:
            cell('cheap', code, prec, cheap, 64, 64, face, [(face, c) for c in CHEAP_CLIPS])
    cell('uneven', _lib.BF16, 'bf16', weights(9200, 32, 64), 32, 64, 7, [(7, 1)])       # input != hidden: no window
    sd = synth.clstm_state(seed=2)
    real = [_dev(sd[k]) for k in ('Conv1.weight', 'Conv1.bias', 'Conv2.weight', 'Conv2.bias', 'Gates.weight', 'Gates.bias')]
    cell('real', _lib.BF16, 'bf16', real, 1000, 1000, 7, REAL_SHAPES)
    return out


def collect(L):
    plans, refusals = _static(L)
    return {'static': plans, 'refusals': refusals, 'clstm': _clstm(L)}


# ---- the fixture: a text is stored as [head, tail] index pairs of its lines, split at the first ': ' (the blocks of a layer and
# the two 16-bit types share most tails; tail -1: a line without one), which keeps 36 texts of up to 60 lines small
def _encode(got):
    heads, tails = {}, {}
    idx = lambda table, s: table.setdefault(s, len(table))
    line = lambda a, sep, b: [idx(heads, a), idx(tails, b) if sep else -1]
    static = {prec: {k: [e[0], [line(*ln.partition(': ')) for ln in e[1].split('\n')], e[2]] for k, e in shapes.items()}
              for prec, shapes in got['static'].items()}
    return {'heads': list(heads), 'tails': list(tails), 'static': static, 'refusals': got['refusals'], 'clstm': got['clstm']}


def _decode(golden):
    heads, tails = golden['heads'], golden['tails']
    text = lambda pairs: '\n'.join(heads[a] if b < 0 else heads[a] + ': ' + tails[b] for a, b in pairs)
    static = {prec: {k: [e[0], text(e[1]), e[2]] for k, e in shapes.items()} for prec, shapes in golden['static'].items()}
    return {'static': static, 'refusals': golden['refusals'], 'clstm': golden['clstm']}


def check_coverage(got):
    """the recorded set takes every branch of the two planners (so a thinned grid cannot pass silently)"""
    texts = [e[1] for shapes in got['static'].values() for e in shapes.values()]
    for note in NOTE_LINES:
        assert any(note in t for t in texts), note
    fused_l2 = [t for t in texts if 'layer2.1-3: conv1 + ONE fused tail launch' in t]
    chained = [t for t in fused_l2 if '  layer2.2 conv 1x1' not in t]
    assert chained and len(chained) < len(fused_l2)             # layer2's tails with and without the next conv1 riding on them
    l4 = [ln for t in texts for ln in t.split('\n') if ln.startswith('  layer4.') and ' conv 3x3 ' in ln]
    assert any('conv_clip' in ln for ln in l4) and any('conv_small' in ln for ln in l4)
    cam = [int(m.group(1)) for t in texts for m in re.finditer(r'(?m)^  CAM conv .* split-K (\d+)', t)]
    assert len(cam) == len(texts) and 1 in cam and max(cam) > 1, sorted(set(cam))
    assert all(e[0] == len(e[1]) and e[2] > 0 for shapes in got['static'].values() for e in shapes.values())
    for r in got['refusals'].values():
        rc, text = r['describe into 16 bytes']
        assert rc == 15 and len(text) == 15 and all(v <= 0 for k, v in r.items() if k != 'describe into 16 bytes'), r
    states = {e[0] for e in got['clstm'].values()}
    assert states == {0, 1, 2}, states
    assert any(k.endswith('+ load_wino') and e[0] == 1 for k, e in got['clstm'].items())
    assert got['clstm']['uneven bf16 face 7 clips 1'][2:] == [0, 0]


def _golden():
    return _decode(json.load(open(GOLDEN)))


@pytest.mark.gpu
def test_stage_planner_answers_equal_the_recording():
    """Entry by entry: the static stage's plan text, its length and workspace size at the twelve shapes in three precisions, the
    status code of every refused call, and the ConvLSTM cell's Winograd state and workspace sizes (before and after
    cp360_clstm_load_wino) are what the library answered before plan_resnet() / plan_clstm()."""
    golden = _golden()
    got = collect(_lib.lib())
    for section in ('static', 'refusals', 'clstm'):
        assert sorted(got[section]) == sorted(golden[section]), section
        for key, want in golden[section].items():
            if section == 'clstm':
                assert got[section][key] == want, (key, got[section][key], want)
                continue
            assert sorted(got[section][key]) == sorted(want), (section, key)
            for k, w in want.items():
                assert got[section][key][k] == w, (section, key, k, got[section][key][k], w)
    n = sum(len(v) for v in golden['static'].values())
    assert n == len(PRECISIONS) * len(STATIC_SHAPES) and len(golden['clstm']) >= 35, (n, len(golden['clstm']))


def test_recording_takes_every_branch_of_the_planners():
    """The fixture is what it claims (no GPU needed): every note line of the static-stage planner, chained and unchained layer2
    tails, clip-resident and small-tile layer4, the CAM with and without split-K, Winograd states 0, 1 and 2."""
    check_coverage(_golden())


if __name__ == '__main__':
    if '--record' not in sys.argv:
        sys.exit(__doc__)
    got = collect(_lib.lib())
    check_coverage(got)
    out = {'recorded_from': sys.argv[sys.argv.index('--record') + 1],
           'format': 'see tests/test_stage_plan.py collect(); a plan text is [head, tail] index pairs of its lines (split at the first ": ")'}
    out.update(_encode(got))
    assert _decode(json.loads(json.dumps(out))) == json.loads(json.dumps(got))          # the encoding round-trips
    with open(GOLDEN, 'w') as f:
        json.dump(out, f, separators=(',', ':'))
    print('%d texts, %d cell entries -> %s (%d bytes)' % (sum(len(v) for v in got['static'].values()), len(got['clstm']), GOLDEN,
                                                          os.path.getsize(GOLDEN)))
