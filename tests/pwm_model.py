"""PwmDecoder (src/pwm_decoder.rs:385-513) restated sample by sample, with a counter per rejection cause, the loader of
tests/golden/pwm_known_answers.json and the fuzz family of pulse trains the CPU and GPU tests share.

PwmModel.process() is the machine, one sample at a time.  push() gives the same result faster: runs of samples that leave the
slicer where it is are taken in one step (the gap events inside a low run by arithmetic on low_run); test_pwm_cpu.py holds it to
process() on the whole fuzz family."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CAUSES = ("invalid_width", "overflow", "wrong_length", "empty", "distinct_cap", "below_min_repeats")

MESSAGES = {
    "high": "PwmDecoder high threshold must be finite and greater than zero",
    "low": "PwmDecoder low threshold must be finite, greater than zero, and no greater than the high threshold",
    "short": "PwmDecoder short pulse width must be greater than zero",
    "long": "PwmDecoder long pulse width must be greater than the short pulse width",
    "frame_gap": "PwmDecoder frame gap must be greater than zero",
    "reset_gap": "PwmDecoder reset gap must be at least as long as the frame gap",
    "frame_bits_zero": "PwmDecoder fixed frame length must be greater than zero",
    "max_frame_bits": "PwmDecoder maximum frame length must be greater than zero",
    "frame_bits_max": "PwmDecoder fixed frame length exceeds the maximum frame length",
    "max_distinct": "PwmDecoder maximum distinct frames must be greater than zero",
    "min_repeats": "PwmDecoder minimum repeats must be greater than zero",
}


class PwmModel:
    def __init__(self, high_threshold, short_width, long_width, frame_gap, reset_gap, *, low_threshold=None, pulse_tolerance=None,
                 frame_bits=None, max_frame_bits=4096, max_distinct_frames=256, min_repeats=1, short_is_one=True, delimiter=False):
        self.high_thr = np.float32(high_threshold)
        self.low_thr = np.float32(self.high_thr / np.float32(2.0)) if low_threshold is None else np.float32(low_threshold)
        self.short, self.long = int(short_width), int(long_width)
        self.tol = abs(self.long - self.short) // 2 if pulse_tolerance is None else int(pulse_tolerance)
        self.fgap, self.rgap = int(frame_gap), int(reset_gap)
        self.frame_bits, self.max_bits, self.max_distinct = frame_bits, int(max_frame_bits), int(max_distinct_frames)
        self.min_repeats, self.short_is_one, self.delimiter = int(min_repeats), bool(short_is_one), bool(delimiter)
        self.validate()
        self.sample_index = 0
        self.high = False
        self.high_run = self.low_run = 0
        self.pending = None
        self.bits = []
        self.frame_start = None
        self.frame_invalid = False
        self.candidates = []                  # [bits, repeats, first_sample]
        self.counters = dict.fromkeys(CAUSES, 0)
        self.max_repeats_seen = 0
        self.reset_samples = []               # the samples at which finish_transmission ran

    def validate(self):                       # :101-162, in its order
        hi, lo = float(self.high_thr), float(self.low_thr)
        if not np.isfinite(hi) or hi <= 0.0:
            raise ValueError(MESSAGES["high"])
        if not np.isfinite(lo) or lo <= 0.0 or lo > hi:
            raise ValueError(MESSAGES["low"])
        if self.short == 0:
            raise ValueError(MESSAGES["short"])
        if self.long <= self.short:
            raise ValueError(MESSAGES["long"])
        if self.fgap == 0:
            raise ValueError(MESSAGES["frame_gap"])
        if self.rgap < self.fgap:
            raise ValueError(MESSAGES["reset_gap"])
        if self.frame_bits is not None and self.frame_bits == 0:
            raise ValueError(MESSAGES["frame_bits_zero"])
        if self.max_bits == 0:
            raise ValueError(MESSAGES["max_frame_bits"])
        if self.frame_bits is not None and self.frame_bits > self.max_bits:
            raise ValueError(MESSAGES["frame_bits_max"])
        if self.max_distinct == 0:
            raise ValueError(MESSAGES["max_distinct"])
        if self.min_repeats == 0:
            raise ValueError(MESSAGES["min_repeats"])

    # ---- :429-513
    def _finish_pending_pulse(self):
        if self.pending is None:
            return
        w, self.pending = self.pending, None
        ds, dl = abs(w - self.short), abs(w - self.long)
        sv, lv = ds <= self.tol, dl <= self.tol
        if not sv and not lv:
            self.counters["invalid_width"] += not self.frame_invalid
            return self._invalidate()
        short = ds <= dl if sv and lv else sv
        if len(self.bits) == self.max_bits:
            self.counters["overflow"] += not self.frame_invalid
            return self._invalidate()
        self.bits.append(int(short == self.short_is_one))

    def _invalidate(self):
        self.bits, self.frame_start, self.frame_invalid = [], None, True

    def _clear_frame(self):
        self.bits, self.frame_start, self.frame_invalid, self.pending = [], None, False, None

    def _finish_frame(self):
        if self.frame_invalid or not self.bits or (self.frame_bits is not None and self.frame_bits != len(self.bits)):
            if not self.frame_invalid:
                self.counters["empty" if not self.bits else "wrong_length"] += 1
            return self._clear_frame()
        first = self.frame_start if self.frame_start is not None else self.sample_index
        for c in self.candidates:
            if c[0] == self.bits:
                c[1] += 1
                self.max_repeats_seen = max(self.max_repeats_seen, c[1])
                break
        else:
            if len(self.candidates) < self.max_distinct:
                self.candidates.append([self.bits, 1, first])
            else:
                self.counters["distinct_cap"] += 1
        self._clear_frame()

    def _finish_transmission(self):
        self._clear_frame()
        out = [(tuple(c[0]), c[1], c[2]) for c in self.candidates if c[1] >= self.min_repeats]
        self.counters["below_min_repeats"] += len(self.candidates) - len(out)
        self.candidates = []
        return out

    def process(self, p):
        """one sample -> the frames a reset on it delivers, or None (:385-427)"""
        p = np.float32(p)
        out = None
        if self.high:
            if p >= self.low_thr:
                self.high_run += 1
            else:
                self.high, self.pending, self.high_run, self.low_run = False, self.high_run, 0, 1
        elif p <= self.high_thr:
            self.low_run += 1
            if self.low_run == self.fgap:
                if self.delimiter:
                    self.pending = None
                else:
                    self._finish_pending_pulse()
                self._finish_frame()
            if self.low_run == self.rgap:
                self.reset_samples.append(self.sample_index)
                out = self._finish_transmission()
        else:
            if self.low_run < self.fgap:
                self._finish_pending_pulse()
            else:
                self.pending = None
            self.high, self.high_run, self.low_run = True, 1, 0
            if not self.bits and not self.frame_invalid:
                self.frame_start = self.sample_index
        self.sample_index += 1
        return out

    def push_slow(self, samples):
        out = []
        for p in np.asarray(samples, np.float32):
            out += self.process(p) or []
        return out

    def push(self, samples):
        """process() over the samples -> the frames delivered inside them; runs that leave the slicer alone in one step"""
        x = np.asarray(samples, np.float32)
        n = len(x)
        rises = np.flatnonzero(~(x <= self.high_thr))        # where a low slicer would rise
        falls = np.flatnonzero(~(x >= self.low_thr))         # where a high slicer would fall
        out, i = [], 0
        while i < n:
            if self.high:
                k = np.searchsorted(falls, i)
                j = int(falls[k]) if k < len(falls) else n
                self.high_run += j - i
            else:
                k = np.searchsorted(rises, i)
                j = int(rises[k]) if k < len(rises) else n
                # the gap events among the j - i samples that stay low, in order (the frame first on a shared sample)
                for gap in sorted({self.fgap, self.rgap}):
                    if self.low_run < gap <= self.low_run + (j - i):
                        at = i + gap - self.low_run - 1
                        self.sample_index += at - i
                        self.low_run += at - i
                        i = at
                        out += self.process(x[i]) or []
                        i += 1
                self.low_run += j - i
            self.sample_index += j - i
            i = j
            if i < n:
                out += self.process(x[i]) or []
                i += 1
        return out

    def flush(self):
        """EOF (:612-618)"""
        return self._finish_transmission()


# ---- the reference's own tests as data ---------------------------------------------------------------------------------------------
def load_known_answers():
    with open(os.path.join(HERE, "golden", "pwm_known_answers.json")) as f:
        return json.load(f)


def golden_samples(doc, case):
    """the add_run / add_frame calls of a case -> f32 samples (:696-712)"""
    k = doc["constants"]
    runs = []
    for op in case["ops"]:
        if op[0] == "run":
            runs.append((bool(op[1]), int(op[2])))
        else:
            for b in op[1]:
                short = b == "1"
                runs.append((True, k["short"] if short else k["long"]))
                runs.append((False, k["long"] if short else k["short"]))
            if op[2] == "Delimiter":
                runs.append((True, k["short"]))
            runs.append((False, k["frame_gap"]))
    return np.concatenate([np.full(c, 1.0 if h else 0.0, np.float32) for h, c in runs] or [np.zeros(0, np.float32)])


def golden_settings(doc, s):
    """a case's builder calls -> the keyword arguments PwmModel and rr.PwmDecoder share"""
    k = dict(doc["builder"]) if s.get("base", "builder") == "builder" else dict(doc["plain"])
    k.update({a: b for a, b in s.items() if a != "base"})
    if isinstance(k.get("low_threshold"), str):
        k["low_threshold"] = float(k["low_threshold"])
    pos = [k.pop(a) for a in ("high_threshold", "short_width", "long_width", "frame_gap", "reset_gap")]
    return pos, k


# ---- the fuzz family -------------------------------------------------------------------------------------------------------------------
FUZZ_SEEDS = range(24)


def fuzz_case(seed):
    """-> (positional settings, keyword settings, f32 samples): a pulse train with jittered widths (the tie |w - short| ==
    |w - long| included), samples exactly on either threshold, inside the hysteresis band, NaN and +-Inf, gaps one below, at and
    one above frame_gap and reset_gap, and reset_gap == frame_gap in every fourth case"""
    rng = np.random.default_rng(1000 + seed)
    short = int(rng.integers(2, 6))
    long = short + 2 * int(rng.integers(1, 4))              # even distance: a width exactly in the middle exists
    tol = (long - short) // 2 if seed % 3 else int(rng.integers(0, long - short))
    fgap = long + int(rng.integers(2, 6))
    rgap = fgap if seed % 4 == 0 else fgap + int(rng.integers(1, 12))
    nbits = int(rng.integers(3, 7))
    kw = dict(pulse_tolerance=tol, low_threshold=0.25 if seed % 5 else 0.5, frame_bits=nbits if seed % 2 else None,
              max_frame_bits=nbits + 1 if seed % 3 == 0 else 16, max_distinct_frames=2 if seed % 6 < 2 else 8,
              min_repeats=1 + seed % 3, short_is_one=bool(seed % 7 != 3), delimiter=bool(seed % 2))
    hi_vals = [1.0, 1.0, 1.0, 0.25 if seed % 5 else 0.5, 0.3 if seed % 5 else 0.5, np.inf, 0.5000001]
    lo_vals = [0.0, 0.0, 0.0, 0.5, 0.3 if seed % 5 else 0.1, -np.inf, 0.1]
    x = []

    def run(high, count):
        vals = hi_vals if high else lo_vals
        for _ in range(count):
            x.append(vals[int(rng.integers(0, len(vals)))] if rng.random() < 0.3 else vals[0])

    def frame(bits, last_gap):
        for b in bits:
            w = short if (b == 1) == kw["short_is_one"] else long
            r = rng.random()
            if r < 0.25:
                w += int(rng.integers(-1, 2))
            elif r < 0.30:
                w = (short + long) // 2                       # the tie
            elif r < 0.34:
                w += int(rng.choice([-tol - 1, tol + 1]))
            run(True, max(w, 1))
            run(False, int(rng.integers(1, fgap)))            # up to one below frame_gap
        if kw["delimiter"]:
            run(True, short)
        run(False, last_gap)

    run(False, int(rng.integers(0, rgap + 3)))
    for _ in range(int(rng.integers(3, 7))):                 # transmissions
        words = [list(rng.integers(0, 2, nbits)) for _ in range(int(rng.integers(1, 4)))]
        seq = [words[int(rng.integers(0, len(words)))] for _ in range(int(rng.integers(1, 7)))]
        if rng.random() < 0.3:
            seq.insert(int(rng.integers(0, len(seq) + 1)), list(rng.integers(0, 2, nbits + int(rng.integers(1, 4)))))
        for q, bits in enumerate(seq):
            end = q == len(seq) - 1
            gaps = [rgap - 1, rgap, rgap + 1] if end else [fgap, fgap + 1, fgap, rgap - 1 if rgap - 1 >= fgap else fgap]
            frame(bits, gaps[int(rng.integers(0, len(gaps)))])
        if rng.random() < 0.25:
            x.append(np.nan)
            run(False, 2)
            x.append(np.nan)
            x.append(np.nan)
    run(True, int(rng.integers(0, 4)))                        # the stream may end inside a pulse
    return [0.5, short, long, fgap, rgap], kw, np.array(x, np.float32)
