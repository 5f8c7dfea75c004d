"""What the GPU tests of rr.AmDemod share: one push through sentinel-filled device buffers with everything beyond the count
checked, a stream taken through a handle in given pushes, and the launch counter."""
import numpy as np
import torch

import am_model as am
import rustradio_amd as rr
from symsync_dev import SENTINEL, u32


def launches():
    return int(rr.lib().rr_debug_kernel_launches())


def dev_push(h, x, in_pad=3, out_pad=5):
    """one rr_am_demod_push_dev of the rows of x (nstreams x n, Complex) into a sentinel-filled device buffer
    -> float32[nstreams, produced]; asserts the count rule and that nothing at or beyond the count was written.  The input's
    padding is NaN: a kernel that read it into an output would show."""
    x = np.ascontiguousarray(x, np.complex64)
    x = x.reshape(1, -1) if x.ndim == 1 else x
    ns, n = x.shape
    want = am.count(h.total + n, h.interp, h.deci) - am.count(h.total, h.interp, h.deci)
    in_stride, out_stride = n + in_pad, want + out_pad
    hin = np.full((ns, in_stride), np.nan + 1j * np.nan, np.complex64)
    hin[:, :n] = x
    d_in = torch.from_numpy(hin.view(np.float32)).cuda()
    d_out = torch.from_numpy(np.full((ns, out_stride), SENTINEL, np.float32)).cuda()
    torch.cuda.synchronize()
    k = h.push_dev(d_in.data_ptr(), in_stride, n, d_out.data_ptr(), out_stride)      # (the count is there before anything ran)
    assert k == want
    h.sync()
    out = d_out.cpu().numpy()
    assert np.all(u32(out[:, k:]) == u32(SENTINEL)), "written at or beyond the count"
    return out[:, :k].copy()


def run_pushes(h, x, lens, **kw):
    """the rows of x through h in pushes of `lens` samples -> float32[nstreams, total produced]"""
    x = np.ascontiguousarray(x, np.complex64)
    x = x.reshape(1, -1) if x.ndim == 1 else x
    assert sum(lens) == x.shape[1]
    parts, at = [], 0
    for n in lens:
        parts.append(dev_push(h, x[:, at:at + n], **kw))
        at += n
    return np.concatenate(parts, axis=1)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(u32(a), u32(b))
