"""What the drivers of the video and evaluation kernels (stabilize, viewport, shots, eval_sphere, fixations, optical_flow) share:
how a caller's array reaches the device, and the table workspace kept per image size."""
import numpy as np
import torch

from .. import ops


def host_tensor(a, np_dtype=None):
    """A tensor as it is; anything numpy reads as a tensor over a contiguous array (of np_dtype when one is given)."""
    return a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, dtype=np_dtype))


def on_device(a, device, dtype=None):
    """A numpy array or a tensor -> a contiguous tensor on `device`, of `dtype` when one is given."""
    a = host_tensor(a)
    return (a.to(device) if dtype is None else a.to(device, dtype)).contiguous()


class TabWork:
    """The table workspace (``ops._stab_work(0, h, w)``) of every image size a driver has met: ``work(t)`` for a tensor t
    [N, h, w, ..] on the device (its own ``device``, with the index: a workspace is kept while it lies there)."""

    def __init__(self):
        self._work = {}

    def __call__(self, t):
        h, w = int(t.shape[1]), int(t.shape[2])
        work = self._work[(h, w)] = ops._stab_work(0, h, w, t.device, self._work.get((h, w)))
        return work
