"""bench.py --dump-outputs on the CPU: which step's outputs are written (run_workload with a stand-in engine whose maps
change from call to call and whose output buffer is overwritten, as the real engine's are) and how an output above
the size budget is sampled (dump_outputs)."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import bench  # noqa: E402


class CountingStub(bench.StubEngine):
    """StubEngine whose map of call i is the stub's map + 1000 i, written into ONE reused buffer."""

    def __init__(self, *a):
        super().__init__(*a)
        self.calls = 0
        self.buf = None

    def __call__(self, frames):
        m = super().__call__(frames) + 1000.0 * self.calls
        self.calls += 1
        if self.buf is None:
            self.buf = torch.empty_like(m)
        self.buf.copy_(m)
        return self.buf


@pytest.mark.parametrize('pipelined', [True, False])
@pytest.mark.parametrize('full', [False, True])
def test_dump_is_the_last_timed_step(monkeypatch, pipelined, full):
    """The dumped maps are those of the K-th timed step (call W + K - 1), also when the --full passes that follow the timed
    region (the one-by-one steps, the all-gather alone) run the engine again and overwrite its buffer."""
    made = []
    monkeypatch.setattr(bench, 'StubEngine', lambda *a: made.append(CountingStub(*a)) or made[-1])
    B, T, W, K = 2, 3, 2, 4
    res = bench.run_workload(torch.device('cpu'), 0, 1, 64, 128, 64, B, T, 'fp32', K, W, stub=True, pipelined=pipelined,
                             want_sequential=full, want_allgather=full, want_outputs=True)
    eng = made[0]
    assert eng.calls == W + K + (K + 2 if full and pipelined else 1 if full else 0)
    frames = torch.stack([torch.from_numpy(bench.synth.clip_u8(3 + b, T, 64, 128)) for b in range(B)])
    want = (bench.StubEngine(64, B, T)(frames) + 1000.0 * (W + K - 1)).numpy()
    got = res['outputs']['saliency']
    assert list(res['outputs']) == ['saliency'] and got.dtype == np.float32 and got.shape == (B, 4, 8)
    assert np.array_equal(got, want)


def test_dump_outputs_samples_an_oversized_array(tmp_path, monkeypatch):
    """An array above its share of the budget is written as a seeded sample of its flat elements plus the flat indices
    (float64); the files stay within the budget, a smaller array and a float64 one are written whole and in their type,
    and a second call writes the same bytes."""
    assert bench.DUMP_BYTES + 3 * 128 <= 64 * 10 ** 6          # the real budget, .npy headers included
    monkeypatch.setattr(bench, 'DUMP_BYTES', 3 * 40000)
    rng = np.random.RandomState(5)
    arrays = {'cam': rng.rand(25, 4000).astype(np.float32), 'small': rng.rand(3, 7).astype(np.float32),
              'wide': rng.rand(11)}
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), arrays)
    files = sorted(os.listdir(tmp_path / 'a'))
    assert files == ['cam.npy', 'cam_index.npy', 'small.npy', 'wide.npy'] and sorted(os.listdir(tmp_path / 'b')) == files
    for f in files:
        assert (tmp_path / 'a' / f).read_bytes() == (tmp_path / 'b' / f).read_bytes(), f
    assert sum(os.path.getsize(tmp_path / 'a' / f) for f in files) <= bench.DUMP_BYTES + len(files) * 128
    idx = np.load(tmp_path / 'a' / 'cam_index.npy')
    cam = np.load(tmp_path / 'a' / 'cam.npy')
    assert idx.dtype == np.float64 and cam.dtype == np.float32 and idx.shape == cam.shape and 1000 < idx.size < 100000
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < 100000 and np.array_equal(idx, np.rint(idx))
    assert np.array_equal(cam, arrays['cam'].reshape(-1)[idx.astype(np.int64)])
    assert np.array_equal(np.load(tmp_path / 'a' / 'small.npy'), arrays['small'])
    wide = np.load(tmp_path / 'a' / 'wide.npy')
    assert wide.dtype == np.float64 and np.array_equal(wide, arrays['wide'])
