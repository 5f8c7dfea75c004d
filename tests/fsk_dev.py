"""What the GPU tests of rr.FskTx share: one push through sentinel-filled device buffers with everything at and beyond the counts
checked on the device, a stream of bits taken through a handle in given pushes, and the launch counter."""
import numpy as np
import torch

import rustradio_amd as rr

SENT_BITS = 0x7fc12345                         # a NaN no kernel of the block can produce, in every f32 of the buffers
PAD = 64                                      # elements behind the counts that must stay untouched


def launches():
    return int(rr.lib().rr_debug_kernel_launches())


def _sentinel(n):
    return torch.full((max(n, 1),), SENT_BITS, dtype=torch.int32, device="cuda")


def dev_push(h, bits, audio=True, keep=True):
    """one rr_fsk_tx_push_dev of `bits` -> (out complex64 tensor on the device, audio float32 tensor or None, launches); asserts the
    counts against rr_fsk_tx_count and that nothing at or beyond them was written.  keep=False: the tensors are not returned."""
    bits = np.ascontiguousarray(bits, np.uint8)
    na, no = h.count(len(bits))
    d_bits = torch.from_numpy(bits.copy()).cuda() if len(bits) else torch.zeros(1, dtype=torch.uint8, device="cuda")
    d_out = _sentinel(2 * (no + PAD))
    d_aud = _sentinel(na + PAD) if audio else None
    torch.cuda.synchronize()
    l0 = launches()
    got = h.push_dev(d_bits.data_ptr() if len(bits) else 0, len(bits), d_out.data_ptr(), no, d_aud.data_ptr() if audio else 0,
                     na if audio else 0)
    assert got == (no, na)                     # (the counts are there before anything ran)
    nl = launches() - l0
    h.sync()
    assert bool((d_out[2 * no:] == SENT_BITS).all()), "out written at or beyond the count"
    if audio:
        assert bool((d_aud[na:] == SENT_BITS).all()), "audio written at or beyond the count"
    out = d_out[:2 * no].view(torch.float32).view(torch.complex64) if no else torch.zeros(0, dtype=torch.complex64, device="cuda")
    aud = d_aud[:na].view(torch.float32) if audio else None
    return out, aud, nl


def run_pushes(h, bits, lens, audio=True):
    """`bits` through h in pushes of `lens` -> (out complex64[], audio float32[] or None, [launches per push]) on the host"""
    assert sum(lens) == len(bits)
    outs, auds, nls, at = [], [], [], 0
    for n in lens:
        o, a, nl = dev_push(h, bits[at:at + n], audio)
        outs.append(o.cpu().numpy())
        if audio:
            auds.append(a.cpu().numpy())
        nls.append(nl)
        at += n
    return np.concatenate(outs), (np.concatenate(auds) if audio else None), nls


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))
