"""The middle of the burst receivers as sequential models: BurstTagger's comparison (src/burst_tagger.rs:68-85), StreamToPdu
(src/stream_to_pdu.rs:198-275) and Midpointer (src/wpcr.rs:62-78).

Two statements of StreamToPdu that share no code:

  StreamToPduSeq   the reference's state machine (Unsync / Packet / Tail) over ARBITRARY tags, `Both` included, one work() call
                   per window, the state kept between calls
  closed_form      what the machine does when the tags are BurstTagger's (strictly alternating, the first one rising): a
                   rule over the rising edges r_j and their falling edges f_j with one carried number, `free` — the formulation
                   the device block resolves in parallel

and two of Midpointer: the reference's (an f32 sum in order) and the device block's (the exactly rounded sum, two ranks of the
total order instead of a partition and two sorts).
"""
import math

import numpy as np

F32 = np.float32
NONE, START, END, BOTH = 0, 1, 2, 3


def burst_tags(trigger, threshold, last=False):
    """BurstTagger over one window -> ([(pos, bool)], last): a tag wherever cur = trigger > threshold differs from the previous
    sample's (burst_tagger.rs:75-83)"""
    tags = []
    thr = F32(threshold)
    for i, tv in enumerate(np.asarray(trigger, F32)):
        cur = bool(tv > thr)
        if cur != last:
            tags.append((i, cur))
        last = cur
    return tags, last


class StreamToPduSeq:
    """stream_to_pdu.rs:198-275, one work() per window.  A PDU is (first, samples): `first` is the absolute stream position of its
    first sample (the reference does not record it; None for an empty PDU), `samples` a list."""

    def __init__(self, max_size, tail):
        self.max_size, self.tail = max_size, tail
        self.state = ("unsync",)
        self.pos = 0                    # samples of the stream so far
        self.out = []

    def _len(self):
        return 0 if self.state[0] == "unsync" else len(self.state[1])

    def _file(self, first, p):
        if len(p) > self.max_size:      # file_burst :113-115
            return
        self.out.append((first if p else None, list(p)))

    def work(self, samples, tags):
        """tags: (pos, bool) with window-relative positions, any number per position -> the PDUs this call pushed"""
        self.out = []
        at = {}
        for pos, val in tags:
            at[pos] = at.get(pos, 0) | (1 if val else 2)
        for i, s in enumerate(samples):
            tv = at.get(i, NONE)
            st = self.state
            if st[0] == "unsync":
                if tv in (NONE, END):
                    new = ("unsync",)
                elif tv == START:
                    new = ("packet", [s], self.pos + i)
                else:                   # Both
                    if self.tail > 0:
                        new = ("tail", [s], self.pos + i, self.tail - 1)
                    else:
                        self._file(None, [])
                        new = ("unsync",)
            elif st[0] == "packet":
                p, first = st[1], st[2]
                if tv in (START, NONE):
                    p.append(s)
                    new = ("packet", p, first)
                else:                   # Both | End
                    tail = self.tail
                    if tail > 0:
                        p.append(s)
                        tail -= 1
                    if tail > 0:
                        new = ("tail", p, first, tail)
                    else:
                        self._file(first, p)
                        new = ("unsync",)
            else:                       # tail: burst tags are ignored
                p, first, tail = st[1], st[2], st[3]
                if tail > 0:
                    p.append(s)
                    tail -= 1
                if tail == 0:
                    self._file(first, p)
                    new = ("unsync",)
                else:
                    new = ("tail", p, first, tail)
            self.state = new
            if self._len() > self.max_size:
                self.state = ("unsync",)
        self.pos += len(samples)
        return self.out


def stream_to_pdu_seq(samples, trigger, threshold, max_size, tail, splits=()):
    """BurstTagger -> StreamToPduSeq over a stream cut at `splits` -> per window the list of (first, samples)"""
    cuts = [0] + sorted(splits) + [len(samples)]
    m, last, per = StreamToPduSeq(max_size, tail), False, []
    for a, b in zip(cuts[:-1], cuts[1:]):
        tags, last = burst_tags(trigger[a:b], threshold, last)
        per.append(m.work(list(samples[a:b]), tags))
    return per


def edges_of(trigger, threshold):
    """the whole stream's edges as two arrays: rising positions, falling positions (len(rising) - len(falling) is 0 or 1)"""
    with np.errstate(invalid="ignore"):
        cur = np.asarray(trigger, F32) > F32(threshold)
    d = np.flatnonzero(np.diff(np.concatenate([[False], cur]).astype(np.int8)))
    return d[0::2], d[1::2]


def closed_form(n, rising, falling, max_size, tail):
    """-> [(start, end, done)]: the PDUs [start, end) of a stream of n samples and the number of samples of the stream that must
    have arrived for each to be pushed (its falling edge and its last sample)"""
    out, free = [], 0
    for j, r in enumerate(rising):
        if r < free or j >= len(falling):
            continue                    # ignored with its falling edge; or still open at the end of the stream
        f = falling[j]
        if (f - r) + tail <= max_size:
            free = f + tail
            if free <= n:
                out.append((int(r), int(f + tail), int(max(f + 1, f + tail))))
        else:
            free = r + max_size + 1
    return out


def closed_form_windows(samples, trigger, threshold, max_size, tail, splits=()):
    """closed_form over the whole stream, its PDUs dealt to the window that completes them -> per window [(first, samples)]"""
    n = len(samples)
    r, f = edges_of(trigger, threshold)
    cuts = [0] + sorted(splits) + [n]
    per = [[] for _ in cuts[1:]]
    for s, e, done in closed_form(n, r, f, max_size, tail):
        w = next(k for k, c in enumerate(cuts[1:]) if done <= c)
        per[w].append((s, list(samples[s:e])))
    return per


# ---- Midpointer -------------------------------------------------------------------------------------------------------------------------
def total_key(x):
    """the order of f32::total_cmp as unsigned integers"""
    u = np.ascontiguousarray(x, F32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def total_sort(x):
    x = np.ascontiguousarray(x, F32)
    return x[np.argsort(total_key(x), kind="stable")]


def midpointer_ref(v):
    """wpcr.rs:62-78 as written: the f32 sum in order, a partition, two sorts -> (mean, offset) or (mean, None) when nothing is
    pushed"""
    v = np.ascontiguousarray(v, F32)
    with np.errstate(all="ignore"):
        acc = np.cumsum(v, dtype=F32)[-1]          # (a running sum: f32, in order)
        mean = F32(acc / F32(len(v)))
        if np.isnan(mean):
            return mean, None
        sel = v > mean
        a, b = total_sort(v[sel]), total_sort(v[~sel])
        if len(a) == 0 or len(b) == 0:
            return mean, None
        high, low = a[len(a) // 2], b[len(b) // 2]
        return mean, F32(low + F32(F32(high - low) / F32(2.0)))


def mean_exact(v):
    """fl32(S / len), S the exactly rounded f64 sum (NaN / Inf as IEEE addition gives them)"""
    v64 = np.ascontiguousarray(v, F32).astype(np.float64)
    if not np.all(np.isfinite(v64)):
        with np.errstate(all="ignore"):
            return F32(np.sum(v64) / len(v64))
    return F32(math.fsum(v64) / len(v64))


def midpointer_block(v, mean=None):
    """the device block's statement from a given mean (default: mean_exact) -> dict(ok, mean, mid, nlow, low, high)"""
    v = np.ascontiguousarray(v, F32)
    mean = mean_exact(v) if mean is None else F32(mean)
    n = len(v)
    if np.isnan(mean):
        return dict(ok=0, mean=mean, mid=F32(0), nlow=n, low=None, high=None)
    with np.errstate(invalid="ignore"):
        nlow = int(np.count_nonzero(~(v > mean)))
    if nlow == 0 or nlow == n:
        return dict(ok=0, mean=mean, mid=F32(0), nlow=nlow, low=None, high=None)
    s = total_sort(v)
    low, high = s[nlow // 2], s[nlow + (n - nlow) // 2]
    with np.errstate(all="ignore"):
        mid = F32(low + F32(F32(high - low) / F32(2.0)))
    return dict(ok=1, mean=mean, mid=mid, nlow=nlow, low=low, high=high)


def noisy_nrz_burst(rng, n, sps, offset, noise):
    """n samples of random NRZ at `sps` samples per symbol around `offset`, with Gaussian noise"""
    nsym = int(n / sps) + 2
    bits = rng.integers(0, 2, nsym) * 2.0 - 1.0
    idx = np.minimum((np.arange(n) / sps).astype(int), nsym - 1)
    return (bits[idx] + offset + noise * rng.standard_normal(n)).astype(F32)
