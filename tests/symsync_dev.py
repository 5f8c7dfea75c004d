"""What the GPU tests of rr.SymbolSync share: one push through sentinel-filled device buffers with everything around the produced
elements checked, and a download of raw device memory."""
import numpy as np
import torch

SENTINEL = np.array([0x7fc12345], np.uint32).view(np.float32)[0]      # a NaN no kernel of the block can produce


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def dev_push(h, x, in_stride=None, out_stride=None, clock=True):
    """one rr_symbol_sync_push_dev of the rows of x (nstreams x n) into sentinel-filled device buffers -> (counts, [symbols of row
    c], [clock values of row c] or None); asserts that nothing outside the produced elements was written and that the counts on the
    device are the ones produced() reports"""
    x = np.ascontiguousarray(x, np.float32)
    x = x.reshape(1, -1) if x.ndim == 1 else x
    ns, n = x.shape
    in_stride = n if in_stride is None else in_stride
    out_stride = n if out_stride is None else out_stride
    hin = np.full((ns, max(in_stride, 1)), 1.0, np.float32)           # (padding of +1.0: a kernel that read it would see sign changes)
    hin[:, :n] = x
    d_in = torch.from_numpy(hin).cuda()
    d_syms = torch.from_numpy(np.full((ns, max(out_stride, 1)), SENTINEL, np.float32)).cuda()
    d_clk = d_syms.clone() if clock else None
    torch.cuda.synchronize()
    h.push_dev(d_in.data_ptr(), in_stride, n, d_syms.data_ptr(), d_clk.data_ptr() if clock else None, out_stride)
    counts = h.produced()                                              # waits for the push
    assert np.array_equal(np.frombuffer(_dev_bytes(h.counts_dev(), 8 * ns), np.uint64), counts)
    syms, clk = d_syms.cpu().numpy(), d_clk.cpu().numpy() if clock else None
    out_s, out_c = [], []
    for c in range(ns):
        k = int(counts[c])
        assert k <= n
        for a, dst in ((syms, out_s), (clk, out_c)):
            if a is None:
                continue
            assert np.all(u32(a[c, k:]) == u32(SENTINEL)), "written beyond the count"
            dst.append(a[c, :k].copy())
    return counts, out_s, out_c if clock else None


class _DevMem:
    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}


def _dev_bytes(ptr, nbytes):
    assert ptr
    return torch.as_tensor(_DevMem(ptr, nbytes), device="cuda").cpu().numpy().tobytes()
