"""Delay (src/delay.rs:62-111) and the sample-rate path of examples/burst_saver.rs:111-131 as sequential models.  Test
infrastructure only: the product never imports it.

  DelaySeq       Delay's work() line by line: the loop, the three return points, eof; `skip` stays 0 (set_delay is not offered)
  delay_model    one work() call per (window, out_cap) pair on a DelaySeq
  SaverSeq       burst_model.mag2_f32 -> iir_ref_f32 -> pdu_model.burst_tags on the trigger branch, DelaySeq on the data branch,
                 pdu_model.StreamToPduSeq behind them: per push the PDUs (first, samples) and the tags; the edges can be given
                 instead (the device's own), which leaves Delay and StreamToPdu as what is modelled
"""
import numpy as np

import burst_model as bm
import pdu_model as pm

WAIT_SRC, WAIT_DST = 1, 2           # RR_WAIT_SRC, RR_WAIT_DST


class DelaySeq:
    def __init__(self, delay, zero=0):
        self.delay = self.current_delay = delay
        self.zero = zero            # T::default()
        self.src = []               # the ReadStream: what has been written and not consumed

    def eof(self, src_eof):
        return self.current_delay == 0 and src_eof and not self.src        # delay.rs:56-60 (src.eof(): closed AND empty)

    def work(self, out_cap):
        """-> (status, consumed, produced, need, out): one work() with `out_cap` free elements in the output stream"""
        out, consumed = [], 0
        while True:
            inp = self.src                                  # :66
            if len(out) == out_cap:                         # :79-82  o.is_empty()
                return WAIT_DST, consumed, len(out), 1, out
            if self.current_delay > 0:                      # :85-91
                n = min(self.current_delay, out_cap - len(out))
                out += [self.zero] * n
                self.current_delay -= n
                continue
            if not inp:                                     # :94-96
                return WAIT_SRC, consumed, len(out), 1, out
            n = min(len(inp), out_cap - len(out))           # :98-109
            assert n != 0
            out += inp[:n]
            del inp[:n]
            consumed += n


def delay_model(windows, delay, out_caps, zero=0):
    """work() once per pair: the window is what the input stream holds at that call (what the previous call left unconsumed is
    dropped: the caller re-offers it, as the C ABI's callers do) -> [(status, consumed, produced, need, out)]"""
    m, res = DelaySeq(delay, zero), []
    for w, cap in zip(windows, out_caps):
        m.src = list(w)
        res.append(m.work(cap))
    return res


def delayed(x, delay, zero=0):
    """the first len(x) outputs of Delay fed x, through the model"""
    m = DelaySeq(delay, zero)
    m.src = list(x)
    return m.work(len(x))[4]


class SaverSeq:
    def __init__(self, alpha, threshold, delay, max_size, tail):
        self.alpha, self.thr = alpha, threshold
        self.prev, self.last = np.float32(0.0), False
        self.delay = DelaySeq(delay, np.complex64(0))
        self.pdu = pm.StreamToPduSeq(max_size, tail)

    def push(self, x, tags=None):
        """-> (PDUs [(first, samples)], tags [(pos, bool)], envelope)"""
        x = np.asarray(x, np.complex64)
        env, self.prev = bm.iir_ref_f32(bm.mag2_f32(x), self.alpha, self.prev)
        if tags is None:
            tags, self.last = pm.burst_tags(env, self.thr, self.last)
        self.delay.src += list(x)
        st, consumed, produced, need, d = self.delay.work(len(x))
        assert produced == len(x)
        return self.pdu.work(d, tags), tags, env
