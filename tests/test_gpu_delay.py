"""GPU: rr_delay (kernels_saver.hip k_delay) against tests/saver_model.py DelaySeq — Delay's work() line by line — at every call:
status, consumed, produced, need, the bytes written, eof; the tag rule and the refusals."""
import numpy as np
import pytest
import torch

import rustradio_amd as rr
import saver_model as sm

pytestmark = pytest.mark.gpu


def payload(n, dtype, seed):
    """n elements of random BITS: NaNs with every payload among the f32 and Complex ones, and at least one for certain"""
    dt = np.dtype(dtype)
    raw = np.random.default_rng(seed).integers(0, 256, n * dt.itemsize, dtype=np.uint8)
    if dt.itemsize >= 4 and n:
        raw.view(np.uint32)[::5] = 0x7FA12345          # a signalling NaN with a payload
    return raw.view(dt)


def as_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


def caps_for(delay, w):
    """several calls that emit only zeros, none at all, one that ends inside the copy, then room for everything"""
    third = delay // 3
    caps = [third, third, 0] if third else [0]
    caps += [delay - 2 * third + (w + 1) // 2]         # what is left of the delay and half a window
    return caps + [w + 5] * 4 + [0, 3 * w + delay + 9]


def drive(b, m, data, w, caps, work):
    pos = 0
    for k, cap in enumerate(caps):
        offered = data[pos:pos + w]
        m.src = list(range(pos + 1, pos + len(offered) + 1))      # the model moves labels: 0 is T::default()
        want = m.work(cap)
        st, c, p, need, out = work(offered, cap)
        assert (st, c, p, need) == want[:4], (k, cap, (st, c, p, need), want[:4])
        lab = np.array(want[4], np.int64)
        ref = np.zeros(len(lab), data.dtype)
        ref[lab > 0] = data[lab[lab > 0] - 1]
        assert np.array_equal(as_bytes(out), as_bytes(ref)), (k, cap)
        assert b.eof(True) == (m.current_delay == 0) and not b.eof(False)
        pos += c
    return pos


@pytest.mark.parametrize("delay", [0, 1, 2047, 2048, 2049])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32, np.complex64])
def test_every_call_against_the_model(dtype, delay):
    for w in (1, 7, 4096):
        data = payload(3 * w + 5, dtype, delay + w)
        b, m = rr.Delay(delay, dtype), sm.DelaySeq(delay)
        assert not b.eof(True) or delay == 0
        caps = caps_for(delay, w)
        pos = drive(b, m, data, w, caps, lambda x, cap: b.work(x, cap))
        assert m.current_delay == 0 and (pos == len(data) or w == 1)
        assert b.tag_rule() == (rr.TAGS_SHIFT, delay)
        assert b.name == "Delay"


@pytest.mark.parametrize("dtype", [np.uint8, np.float32, np.complex64])
def test_device_windows(dtype):
    """rr_block_work_dev on device buffers: the slots behind `produced` stay untouched"""
    delay, w = 2049, 4096
    data = payload(3 * w + 5, dtype, 3)
    d_all = torch.from_numpy(as_bytes(data).copy()).cuda()
    es = np.dtype(dtype).itemsize
    b, m = rr.Delay(delay, dtype), sm.DelaySeq(delay)
    state = {"pos": 0}

    def work(x, cap):
        d_out = torch.full(((cap + 3) * es,), 0xAB, dtype=torch.uint8, device="cuda")
        st, c, p, need = b.work_dev(d_all.data_ptr() + state["pos"] * es, len(x), d_out.data_ptr(), cap)
        b.sync()
        h = d_out.cpu().numpy()
        assert np.all(h[p * es:] == 0xAB)
        state["pos"] += c
        return st, c, p, need, h[:p * es].view(dtype)

    drive(b, m, data, w, caps_for(delay, w), work)


def test_refusals():
    n0 = rr.lib().rr_debug_kernel_launches()
    for dt in (np.uint16, np.complex128):
        with pytest.raises(ValueError, match="unsupported element size"):
            rr.Delay(4, dt)
    with pytest.raises(ValueError, match="delay: more than 1,024,000 samples"):
        rr.Delay(1_024_001, np.float32)
    assert rr.lib().rr_debug_kernel_launches() == n0
    b = rr.Delay(1_024_000, np.uint8)                  # the cap itself is taken
    st, c, p, need, out = b.work(np.arange(4, dtype=np.uint8), 6)
    assert (st, c, p, need) == (rr.WAIT_DST, 0, 6, 1) and not out.any()
