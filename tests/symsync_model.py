"""Test infrastructure: the reference's SymbolSync (src/symbol_sync.rs:46-217) with TedZeroCrossing and IirFilter
(src/iir_filter.rs:57-125) as its sequential machine, every operation an np.float32 scalar operation in the reference's order, and
the signals the SymbolSync tests run it on."""
from __future__ import annotations

import warnings

import numpy as np

F = np.float32


class IirFilter:
    """IirFilter<Float> (iir_filter.rs:57-125); buf is the VecDeque, oldest first"""

    def __init__(self, taps):
        assert len(taps) > 0                                   # :68
        self.taps = [F(t) for t in taps]
        self.buf = []

    def fill(self, s):                                         # :96-101
        self.buf = [F(s)] * (len(self.taps) - 1)

    def filter_clamped(self, sample, mi, mx):                  # :113-124
        ret = self.taps[0] * sample
        for i, s in enumerate(reversed(self.buf)):
            ret = ret + s * self.taps[i + 1]
        ret = mi if ret < mi else (mx if ret > mx else ret)    # f32::clamp
        self.buf.append(ret)
        if len(self.buf) == len(self.taps):
            self.buf.pop(0)
        return ret


class SymbolSync:
    """SymbolSync::new(src, sps, max_deviation, TedZeroCrossing, IirFilter::new(taps)) and its work() loop, one call of run() per
    input window; the output always has room.  State is kept from run() to run()."""

    def __init__(self, sps, max_deviation, taps):
        self.sps = F(sps)
        assert self.sps > F(1.0)                               # :78
        self.max_deviation = F(max_deviation)
        self.filter = IirFilter(taps)
        self.filter.fill(self.sps)                             # :79
        self.clock = self.sps
        self.last_sign = False
        self.stream_pos = F(0.0)
        self.last_sym_boundary_pos = F(0.0)
        self.next_sym_middle = self.sps / F(2.0)
        self.max_fold_iters = 0                                # most iterations of the `while t > mx` loop at one sign change
        self.step_backs = 0
        self.clock_updates = 0

    def run(self, samples):
        """-> (symbols float32[], clock values float32[], window-relative indices of the emitted samples int64[])"""
        x = np.ascontiguousarray(samples, np.float32)
        with np.errstate(invalid="ignore"):
            signs = (x > F(0.0)).tolist()                      # :154 (NaN, +-0.0 and -Inf: false)
        idx, clocks = [], []
        sps, one, ten, half = self.sps, F(1.0), F(10.0), F(2.0)
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            for i, sign in enumerate(signs):
                if self.stream_pos >= self.next_sym_middle:                                         # :142-149
                    idx.append(i)
                    clocks.append(self.clock)
                    self.next_sym_middle = self.next_sym_middle + self.clock
                if sign != self.last_sign:                                                          # :155
                    if self.stream_pos > F(0.0) and self.last_sym_boundary_pos > F(0.0):
                        assert self.stream_pos > self.last_sym_boundary_pos                         # :157
                        mi = sps - self.max_deviation
                        mx = sps + self.max_deviation
                        t = self.stream_pos - self.last_sym_boundary_pos
                        it = 0
                        while t > mx:                                                               # :167-173
                            t2 = t - self.clock
                            if abs(t - self.clock) < abs(t2 - self.clock):
                                break
                            t = t2
                            it += 1
                        self.max_fold_iters = max(self.max_fold_iters, it)
                        if t > mi * F(0.8) and t < mx * F(1.2):                                     # :174
                            assert t > F(0.0)                                                       # :175
                            self.clock = self.filter.filter_clamped(t - sps, mi - sps, mx - sps) + sps
                            self.next_sym_middle = self.last_sym_boundary_pos + self.clock / half
                            while self.next_sym_middle < self.stream_pos:
                                self.next_sym_middle = self.next_sym_middle + self.clock
                            self.clock_updates += 1
                    self.last_sym_boundary_pos = self.stream_pos
                    self.last_sign = sign
                self.stream_pos = self.stream_pos + one                                             # :199
                step_back = ten * self.clock
                if self.stream_pos > step_back and self.last_sym_boundary_pos > step_back and self.next_sym_middle > step_back:
                    self.stream_pos = self.stream_pos - step_back
                    self.last_sym_boundary_pos = self.last_sym_boundary_pos - step_back
                    self.next_sym_middle = self.next_sym_middle - step_back
                    self.step_backs += 1
        ii = np.asarray(idx, np.int64)
        return x[ii] if len(ii) else np.zeros(0, np.float32), np.asarray(clocks, np.float32), ii

    def state(self):
        """what rr.SymbolSync.state() reports"""
        return {"clock": F(self.clock), "stream_pos": F(self.stream_pos), "last_sym_boundary_pos": F(self.last_sym_boundary_pos),
                "next_sym_middle": F(self.next_sym_middle), "last_sign": bool(self.last_sign),
                "hist": np.asarray(self.filter.buf, np.float32)}


def states_equal(a, b):
    """two state() dicts, bit for bit"""
    f = ("clock", "stream_pos", "last_sym_boundary_pos", "next_sym_middle")
    return (all(np.float32(a[k]).view(np.uint32) == np.float32(b[k]).view(np.uint32) for k in f) and a["last_sign"] == b["last_sign"]
            and np.array_equal(np.asarray(a["hist"], np.float32).view(np.uint32), np.asarray(b["hist"], np.float32).view(np.uint32)))


def states_match(a, b):
    """states_equal, but a field that is NaN in one must be NaN in the other, whatever its payload and sign bits: IEEE 754 leaves
    the payload of a NaN an operation makes to the implementation, and the device and numpy differ in it"""
    def same(x, y):
        x, y = np.asarray(x, np.float32).ravel(), np.asarray(y, np.float32).ravel()
        nx, ny = np.isnan(x), np.isnan(y)
        return x.shape == y.shape and np.array_equal(nx, ny) and np.array_equal(x.view(np.uint32)[~nx], y.view(np.uint32)[~ny])
    f = ("clock", "stream_pos", "last_sym_boundary_pos", "next_sym_middle", "hist")
    return all(same(a[k], b[k]) for k in f) and a["last_sign"] == b["last_sign"]


def bits_equal(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- the parameter sets of the reference's examples -------------------------------------------------------------------------
AX25_9600 = (50000.0 / 9600.0, 0.1, [0.0001, 0.99999999])      # examples/ax25-9600-rx.rs:186-193
AX25_1200 = (50000.0 / 1200.0, 0.5, [0.0001, 0.99999999])
ADAPTIVE_9600 = (50000.0 / 9600.0, 0.5, [0.1, 0.9])
# ---- the edges of sps: nearly every sample a symbol (the smallest f32 above 1 among them), and a handful of symbols ------------
SPS_EDGES = {"1.25": (1.25, 0.625, [0.5, 0.5]), "1.5": (1.5, 0.75, [0.1, 0.9]), "2": (2.0, 0.0, [1.0]),
             "200": (200.0, 20.0, [0.2, 0.5, 0.3]), "1+ulp": (float(np.nextafter(F(1.0), F(2.0))), 0.5, [0.5, 0.5])}
SPS_EDGE_N = 3000
SPS_EDGE_PUSHES = (1, 63, 64, 65, 0, SPS_EDGE_N - 193)
# taps that overflow at the first clock update: 5 * 3e38 is +Inf, +Inf - Inf is NaN, and f32::clamp hands a NaN through
NONFINITE = (5.0, 0.5, [1.0, 3e38, -3e38])
NONFINITE_N = 1500


# ---- signals ------------------------------------------------------------------------------------------------------------------------
def hold(levels, sps, offset=0.0):
    """every level held over sps * (1 + offset) samples: sample i is levels[floor(i / (sps (1 + offset)))]"""
    lv = np.asarray(levels, np.float32)
    per = float(sps) * (1.0 + offset)
    n = int(np.floor(len(lv) * per))
    k = np.minimum(np.floor(np.arange(n) / per).astype(np.int64), len(lv) - 1)
    return lv[k]


def nrz(nsyms, sps, seed, offset=0.0, smooth=0, noise=0.0):
    """nsyms random NRZ levels (+-1) held over sps (1 + offset) samples each, a moving average over `smooth` samples, Gaussian noise"""
    rng = np.random.default_rng(seed)
    x = hold(np.where(rng.integers(0, 2, nsyms) != 0, 1.0, -1.0), sps, offset).astype(np.float64)
    if smooth > 1:
        x = np.convolve(x, np.ones(smooth) / smooth, mode="same")
    if noise:
        x = x + noise * rng.standard_normal(len(x))
    return x.astype(np.float32)


def sps_edge_signal(key):
    """SPS_EDGE_N samples of noisy NRZ at the symbol length of SPS_EDGES[key], 0.3 % slow"""
    sps = SPS_EDGES[key][0]
    return nrz(int(SPS_EDGE_N / sps) + 8, sps, 40 + len(key), offset=0.003, noise=0.1)[:SPS_EDGE_N]


def nonfinite_signal():
    return nrz(NONFINITE_N // 5 + 8, NONFINITE[0], 63, offset=0.002, noise=0.1)[:NONFINITE_N]


def with_gap(x, at, length):
    """`length` zeros inserted in front of sample `at`"""
    return np.concatenate([x[:at], np.zeros(length, np.float32), x[at:]]).astype(np.float32)


def with_specials(x, seed, count=40):
    """NaN, +-Inf and -0.0 / +0.0 sprinkled over a copy of x"""
    rng = np.random.default_rng(seed)
    y = np.array(x, np.float32)
    vals = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0], np.float32)
    pos = rng.choice(len(y), size=min(count, len(y)), replace=False)
    y[pos] = vals[rng.integers(0, len(vals), len(pos))]
    return y


def sign_words(x):
    """what k_sync_signs leaves for a window: bit b of word w = x[64 w + b] > 0.0, zeros beyond the window"""
    x = np.ascontiguousarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        s = (x > 0).astype(np.uint8)
    s = np.concatenate([s, np.zeros((-len(s)) % 64, np.uint8)])
    return np.packbits(s.reshape(-1, 64), axis=1, bitorder="little").view(np.uint64).ravel() if len(s) else np.zeros(0, np.uint64)
