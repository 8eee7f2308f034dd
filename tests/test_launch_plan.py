"""Planner equivalence on the CPU: what the launch planner of csrc/conv_igemm.hip says about a fixed set of convolution
descriptors (cp360_conv_plan_describe, cp360_conv_suggest_splits, cp360_conv_partial_bytes, cp360_conv_packed_bytes,
cp360_conv_prefer_clip) against tests/golden/conv_plans.json, recorded from the library BEFORE the host side was folded into
resolve_launch().  Every entry must be equal - except the descriptions that named a kernel other than the one
cp360_conv_forward2 launches, which are listed in KNOWN_CORRECTIONS with the reason and asserted against the corrected text.

Recording (against a build of the commit to compare with):
    CP360_LIB=<that build>/libcp360.so python -m tests.test_launch_plan --record <its commit hash>
"""
import ctypes as C
import json
import os
import re
import sys

from cp_360_weakly_supervised_saliency_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'conv_plans.json')
TILES = (0, 64, 128, 129, 160, 256, 304, 6464)
DTYPES = (_lib.F32, _lib.BF16, _lib.F16)
TEXT = re.compile(r'^(.*?), (\d+) workgroups x split-K (\d+)( \(\+ second source\))?, model (\d+) us$')


def _desc(dtype, n_img, face, c_in, c_out, k, stride=1, tile_px=0, clip_resident=0, second=None):
    d = _lib.ConvDesc()
    pad = 1 if k == 3 else 0
    ho = (face + 2 * pad - k) // stride + 1
    for key, v in dict(dtype=dtype, n_img=n_img, h_in=face, w_in=face, c_in=c_in, pix_stride=c_in, kh=k, kw=k, sy=stride, sx=stride,
                       h_out=ho, w_out=ho, c_out=c_out, pad_mode=1 if pad else 0, pad=pad, ld_out=c_out, out_coff=0, ld_res=0,
                       relu=1, splits=1, tile_px=tile_px, clip_resident=clip_resident).items():
        setattr(d, key, v)
    if second:                                                  # the Bottleneck's downsample branch: 1x1, stride 2, from the block input
        d.c_in2, d.pix_stride2, d.h_in2, d.w_in2, d.sy2, d.sx2 = second[0], second[0], second[1], second[1], 2, 2
    return d


def network_shapes(cube):
    """The 22 shapes of tests/test_abi.py::test_launch_planner_over_the_network_shapes."""
    f1 = cube // 4
    return [(f1, 64, 64, 1, 1), (f1, 64, 64, 3, 1), (f1, 64, 256, 1, 1), (f1, 256, 64, 1, 1),
            (f1, 256, 128, 1, 1), (f1, 128, 128, 3, 2), (f1 // 2, 128, 512, 1, 1), (f1 // 2, 512, 128, 1, 1),
            (f1 // 2, 128, 128, 3, 1), (f1 // 2, 512, 256, 1, 1), (f1 // 2, 256, 256, 3, 2), (f1 // 4, 256, 1024, 1, 1),
            (f1 // 4, 1024, 256, 1, 1), (f1 // 4, 256, 256, 3, 1), (f1 // 4, 1024, 512, 1, 1), (f1 // 4, 512, 512, 3, 2),
            (f1 // 8, 512, 2048, 1, 1), (f1 // 8, 2048, 512, 1, 1), (f1 // 8, 512, 512, 3, 1), (f1 // 8, 2048, 1000, 1, 1),
            (f1 // 8, 2000, 4000, 3, 1), (f1 // 8, 4000, 4000, 3, 1)]


def descriptors():
    """(key, descriptor, with_prefer_clip) in a fixed order.  Forced tiles at 1 and 64 frames, the planner's own choice at
    1 / 4 / 16 / 64; every dtype and every tile_px value everywhere."""
    for cube in (224, 256, 512):
        f1 = cube // 4
        # conv3 + downsample of layers 2-4 (second source): (face, c_in, c_out, (c_in2, face of the block input))
        second = [(f1 // 2, 128, 512, (256, f1)), (f1 // 4, 256, 1024, (512, f1 // 2)), (f1 // 8, 512, 2048, (1024, f1 // 4))]
        for dtype in DTYPES:
            for tile in TILES:
                for frames in ((1, 4, 16, 64) if tile == 0 else (1, 64)):
                    for face, cin, cout, k, s in network_shapes(cube):
                        yield ('net', cube, dtype, tile, frames, face, cin, cout, k, s), _desc(dtype, 6 * frames, face, cin, cout, k, s, tile), False
                    for face, cin, cout, sec in second:
                        yield ('second', cube, dtype, tile, frames, face, cin, cout, sec[0]), _desc(dtype, 6 * frames, face, cin, cout, 1, 1, tile, second=sec), False
    for face in (4, 7, 8, 16, 9, 12):                           # clip-resident: accepted at 4, 7, 8, 16, refused at 9, 12
        for clips in (1, 4):
            for dtype in DTYPES:
                for c in (512, 4000):
                    yield ('clip', face, clips, dtype, c), _desc(dtype, 6 * clips, face, c, c, 3, 1, clip_resident=1), True


def query(L, d, prefer):
    """[describe rc, kernel name (+ second-source mark), workgroups, split-K, model us, suggested splits, partial bytes at that
    split count, packed bytes(, prefer_clip)]; [rc, ...] with the text fields left out where describe refuses."""
    buf = C.create_string_buffer(256)
    rc = L.cp360_conv_plan_describe(C.byref(d), buf, 256)
    sp = L.cp360_conv_suggest_splits(C.byref(d))
    d.splits = sp
    tail = [sp, L.cp360_conv_partial_bytes(C.byref(d)), L.cp360_conv_packed_bytes(C.byref(d))]
    d.splits = 1
    if prefer:
        tail.append(L.cp360_conv_prefer_clip(C.byref(d)))
    if rc < 0:
        return [rc] + tail
    text = buf.value.decode()
    m = TEXT.match(text)
    assert m and rc == len(text), (rc, text)
    return [rc, m.group(1) + (m.group(4) or ''), int(m.group(2)), int(m.group(3)), int(m.group(5))] + tail


def _entries():
    """the recording, kernel names put back in place of their index into the fixture's name table"""
    golden = json.load(open(GOLDEN))
    return [[e[0], golden['names'][e[1]]] + e[2:] if e[0] > 0 else e for e in golden['entries']]


# ---- descriptions that named a kernel cp360_conv_forward2 does not launch (read off the code before the refactor; every other
# entry equals the recording).  Each rule: (reason, applies(key, desc), corrected(recorded entry, desc)).
PW64 = 'conv_pw64 64 ch x 16 px blocks, grid-stride (4 waves)'
RING2 = 'conv_igemm_ring2 256 ch x 128 px (two workgroups per CU) (+ second source)'
RING256 = 'conv_igemm_ring 256 ch x 256 px (+ second source)'


def _retext(e, name, wgs):
    """the entry with another kernel name / workgroup count: the return code is the text's length"""
    old = len('%s, %d' % (e[1].replace(' (+ second source)', ''), e[2]))
    new = len('%s, %d' % (name.replace(' (+ second source)', ''), wgs))
    return [e[0] - old + new, name, wgs] + e[3:]


def _m(d):
    return d.n_img * d.h_out * d.w_out


KNOWN_CORRECTIONS = [
    ("a 16-bit 1x1 64 -> 64 convolution with M >= 4096 (layer1.0's conv1) is launched on conv_pw64_kernel with its grid-stride "
     "grid; it was described as the 64 x 256-tile conv_igemm kernel",
     lambda key, d: key[0] == 'net' and d.dtype != _lib.F32 and d.tile_px == 0 and (d.kh, d.c_in, d.c_out, d.sy) == (1, 64, 64, 1) and _m(d) >= 4096,
     lambda e, d: _retext(e, PW64, min(((_m(d) + 15) // 16 + 7) // 8, 2048)), 'conv_igemm 64 ch x 256 px (4 waves)'),
    ("a second-source convolution with a forced tile_px = 128 is launched on the ring2 kernel in the 16-bit types (the DMA "
     "kernel has no second-source loader); it was described as conv_igemm_dma",
     lambda key, d: key[0] == 'second' and d.tile_px == 128 and d.dtype != _lib.F32,
     lambda e, d: _retext(e, RING2, e[2]), 'conv_igemm_dma 256 ch x 128 px (+ second source)'),
    ("... and on the 256-pixel ring in f32, whose grid has 256-pixel tiles",
     lambda key, d: key[0] == 'second' and d.tile_px == 128 and d.dtype == _lib.F32,
     lambda e, d: _retext(e, RING256, (d.c_out + 255) // 256 * ((_m(d) + 255) // 256) * e[3]), 'conv_igemm_dma 256 ch x 128 px (+ second source)'),
    ("a second-source convolution with a forced tile_px = 64 is refused by cp360_conv_forward2 (UNSUPPORTED: the 4-wave "
     "128 x 128 kernel has no second-source loader); it was described as that kernel",
     lambda key, d: key[0] == 'second' and d.tile_px == 64,
     lambda e, d: [-8] + e[5:], 'conv_igemm 128 ch x 128 px (4 waves) (+ second source)'),
    ("a second-source convolution with a forced tile_px = 160 (16-bit) is refused by cp360_conv_forward2 (UNSUPPORTED: only the "
     "256 / 304 rings and ring2 load a second source); it was described as the 160-pixel ring",
     lambda key, d: key[0] == 'second' and d.tile_px == 160 and d.dtype != _lib.F32,
     lambda e, d: [-8] + e[5:], 'conv_igemm_ring 256 ch x 160 px (+ second source)'),
]


def test_planner_answers_equal_the_recording():
    """Entry by entry: describe's return code and text, the suggested split count, the workspace and packed-weight sizes and
    prefer_clip are what the library answered before resolve_launch() - except the KNOWN_CORRECTIONS, where the recording
    holds the wrong kernel name (asserted too, so that a rule cannot hide another difference) and the corrected entry is
    required."""
    L = _lib.lib()
    entries = _entries()
    n, corrected = 0, [0] * len(KNOWN_CORRECTIONS)
    for (key, d, prefer), want in zip(descriptors(), entries):
        n += 1
        for i, (reason, applies, fix, was) in enumerate(KNOWN_CORRECTIONS):
            if applies(key, d):
                assert want[1] == was, (key, want, reason)
                want = fix(want, d)
                corrected[i] += 1
                break
        got = query(L, d, prefer)
        assert got == want, (key, got, want)
    assert n == len(entries) and n > 4000, (n, len(entries))
    assert all(corrected), corrected                            # every rule meets descriptors of the set


def test_recording_holds_refusals_and_every_kernel_family():
    """The fixture is what it claims: clip-resident descriptors at faces 9 / 12 are refused (UNSUPPORTED), faces 4 / 7 / 8 / 16
    accepted on their three tiles, and small, narrow, 128, DMA, ring 160 / 256 / 304 and ring2 tiles all occur."""
    entries = _entries()
    names = set()
    for (key, d, prefer), e in zip(descriptors(), entries):
        if key[0] == 'clip':
            assert (e[0] == -8) == (key[1] in (9, 12)), (key, e)
        if e[0] > 0:
            names.add(e[1].replace(' (+ second source)', ''))
    assert len(names) == 11, sorted(names)


if __name__ == '__main__':
    if '--record' not in sys.argv:
        sys.exit(__doc__)
    L = _lib.lib()
    out = {'recorded_from': sys.argv[sys.argv.index('--record') + 1],
           'format': 'entries in the order of tests/test_launch_plan.py descriptors(): see query(); kernel names as indices into names',
           'entries': [query(L, d, prefer) for key, d, prefer in descriptors()]}
    out['names'] = sorted({e[1] for e in out['entries'] if e[0] > 0})
    out['entries'] = [[e[0], out['names'].index(e[1])] + e[2:] if e[0] > 0 else e for e in out['entries']]
    with open(GOLDEN, 'w') as f:
        json.dump(out, f, separators=(',', ':'))
    print('%d entries -> %s (%d bytes)' % (len(out['entries']), GOLDEN, os.path.getsize(GOLDEN)))
