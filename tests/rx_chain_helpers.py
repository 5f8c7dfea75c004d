"""What the receive-chain tests share (tests/test_gpu_rx_chain.py; the conditions on the signals are asserted on the models alone by
tests/test_rx_chain_cpu.py): the ragged 66-stream input of SymbolSync -> HdlcReceiver, the 5-station FSK band of FmMulti ->
SymbolSync -> HdlcReceiver with its float64 front end, and the chain of Python machines either is held to.  Nothing here touches
the GPU library."""
import functools

import numpy as np

import hdlc_model as hm
import hdlcrx_helpers as hx
import receiver_model as rm
import symsync_model as sm

G3RUH = hx.G3RUH
FIX = 2                                      # rr.HDLC_FIX_BITS

# ---- the ragged signal: SymbolSync(ADAPTIVE_9600, 66) -> HdlcReceiver(66, 1, 60, nrzi, G3RUH) -----------------------------------
RAGGED_N, RAGGED_PRM, RAGGED_MAX_SIZE = 66, sm.ADAPTIVE_9600, 60
ZERO_ROW, GAP_ROW, SPECIALS_ROW = 9, 22, 35  # all zeros; 3,000 zeros inside the second frame; NaN, +-Inf and +-0.0 sprinkled in
FLIPPED_ROWS = (3, 40, 65)                   # the FIX_BITS copy: one bit wrong inside the second frame of each


def ragged_payloads(c):
    rng = np.random.default_rng(500 + c)
    return [rng.integers(0, 256, 12 + 7 * (c % 5), dtype=np.uint8).tobytes() for _ in range(3)]


def _bits(c, flip_at=None):
    bits, k = hm.FLAG * 20, 2 + c % 3
    for i, p in enumerate(ragged_payloads(c)):
        fb = hm.frame_bits(p, k, k)
        if flip_at is not None and i == 1:
            fb[8 * k + flip_at] ^= 1
        bits = bits + fb
    return bits + hm.FLAG * 4


@functools.lru_cache(maxsize=None)
def flip_position(c):
    """the first bit from 41 on of the second frame's stuffed body whose flip the deframer MODEL repairs (3 frames, 1 of them
    repaired).  Most do; one that makes or breaks a run of five ones moves the stuffing or ends the frame, and is passed over."""
    for j in range(41, 90):
        m = hm.HdlcModel(1, RAGGED_MAX_SIZE, False, True)
        m.run(_bits(c, j))
        if m.stats() == (3, 0, 1):
            return j
    raise AssertionError("no repairable bit")


def ragged_bits(c, flipped=False):
    """20 flags, three frames of 12 + 7 (c % 5) random bytes between 2 + c % 3 flags, 4 flags.  flipped: bit flip_position(c) of
    the second frame's stuffed body is wrong.  (The bit is flipped in front of the line coding: behind NrziDecode and the descrambler
    ONE wrong level is six wrong bits, which HDLC_FIX_BITS, a search over single bits, does not repair.)"""
    return _bits(c, flip_position(c) if flipped else None)


def ragged_row(c, flipped=False):
    """stream c before the padding: every level held over sps (1 + offset_c) samples, offset_c = ((5 c) % 13 - 6) 0.0007, a moving
    average over 1 + 2 (c % 2) samples, Gaussian noise of sigma 0.05"""
    if c == ZERO_ROW:
        return np.zeros(64, np.float32)
    lv = hx.line_encode(ragged_bits(c, flipped), nrzi=True, descrambler=G3RUH)
    x = sm.hold(lv, RAGGED_PRM[0], ((5 * c) % 13 - 6) * 0.0007).astype(np.float64)
    w = 1 + 2 * (c % 2)
    if w > 1:
        x = np.convolve(np.concatenate([np.full(w // 2, x[0]), x, np.full(w // 2, x[-1])]), np.ones(w) / w, mode="valid")
    x = (x + 0.05 * np.random.default_rng(900 + c).standard_normal(len(x))).astype(np.float32)
    if c == GAP_ROW:
        # the middle of the second frame: behind 20 + k flags, the first frame and its k closing flags
        k = 2 + c % 3
        first = len(hm.frame_bits(ragged_payloads(c)[0], k, k))
        at = int((160 + first + 8 * k + 17 + 100) * RAGGED_PRM[0])
        x = sm.with_gap(x, at, 3000)
    if c == SPECIALS_ROW:
        x = sm.with_specials(x, 7, 40)
    return x


@functools.lru_cache(maxsize=None)
def ragged_samples(flipped=False):
    """-> f32[66, n], read-only; the shorter rows end in their last level (ZERO_ROW in zeros)"""
    rows = [ragged_row(c, flipped and c in FLIPPED_ROWS) for c in range(RAGGED_N)]
    n = max(len(r) for r in rows)
    last = lambda r: np.sign(r[-1]) if np.isfinite(r[-1]) else 1.0
    x = np.stack([np.concatenate([r, np.full(n - len(r), last(r), np.float32)]) for r in rows])
    x.setflags(write=False)
    return x


def ragged_cuts(n):
    """three pushes: about a third of the samples plus 7, then 64, then the rest"""
    return [n // 3 + 7, 64, n - n // 3 - 7 - 64]


def chain_model(x, cuts, prm, rx_args, rx_kw):
    """sm.SymbolSync(*prm) -> hx.ModelReceiver(*rx_args, **rx_kw) per row of x over the pushes `cuts` -> per push a dict:
    syms [row] f32[], counts [row], frames [row][(pos, bytes, fixed)], stats [row] (3 counters so far), consumed [row] (so far)"""
    syncs = [sm.SymbolSync(*prm) for _ in range(len(x))]
    rxs = [hx.ModelReceiver(*rx_args, **rx_kw) for _ in range(len(x))]
    total, out, at = [0] * len(x), [], 0
    for n in cuts:
        syms = [syncs[c].run(x[c][at:at + n])[0] for c in range(len(x))]
        frames = [rxs[c].push(syms[c]) for c in range(len(x))]
        total = [t + len(s) for t, s in zip(total, syms)]
        out.append({"syms": syms, "counts": [len(s) for s in syms], "frames": frames, "stats": [r.stats() for r in rxs],
                    "consumed": list(total)})
        at += n
    return out


@functools.lru_cache(maxsize=None)
def ragged_model(flags=0):
    """the models over the ragged signal (flags == FIX: over its copy with the three flipped bits) in its three pushes"""
    x = ragged_samples(bool(flags & FIX))
    return chain_model(x, ragged_cuts(x.shape[1]), RAGGED_PRM, (1, RAGGED_MAX_SIZE), dict(nrzi=True, descrambler=G3RUH, flags=flags))


# ---- the FM signal: FmMulti(taps, 1, 10) -> SymbolSync(5.0, 0.5, [0.1, 0.9], 5) -> HdlcReceiver(5, 1, 60, nrzi, G3RUH) ------------------
FM_FS, FM_NCHAN, FM_DECI, FM_DEV_HZ, FM_HOLD, FM_SMOOTH = 480e3, 5, 10, 4.8e3, 50, 20
FM_PRM, FM_MAX_SIZE = (5.0, 0.5, [0.1, 0.9]), 60
FM_RX_KW = dict(nrzi=True, descrambler=G3RUH)


def fm_centres():
    """multiples of the channel rate: they fold to DC behind the 1:10 pick (receiver_model.shape_distinct)"""
    return [(i - 2) * FM_FS / FM_DECI for i in range(FM_NCHAN)]


def fm_taps():
    """a 129-tap low-pass with its cutoff at 0.30 of the channel rate, shifted to every centre -> complex64[5, 129]"""
    return rm.shifted(rm.sinc_low_pass(129, 0.30 / FM_DECI), FM_FS, fm_centres())


def fm_payloads(i):
    rng = np.random.default_rng(700 + i)
    return [rng.integers(0, 256, 12 + 7 * i, dtype=np.uint8).tobytes() for _ in range(3)]


def fm_levels(i):
    """24 flags, three frames of 12 + 7 i bytes between 2 + i flags, 6 flags; G3RUH and NRZI"""
    bits = hm.FLAG * 24
    for p in fm_payloads(i):
        bits = bits + hm.frame_bits(p, 2 + i, 2 + i)
    return hx.line_encode(bits + hm.FLAG * 6, nrzi=True, descrambler=G3RUH)


@functools.lru_cache(maxsize=None)
def fm_samples():
    """-> complex64[n], read-only: station i on centre i, FSK of +-4.8 kHz by channel i's levels held over 50 (1 + (i - 2) 0.002)
    input samples and smoothed over 20, amplitude 1 / 5, plus complex noise of sigma 1e-3"""
    waves = [sm.hold(fm_levels(i), FM_HOLD, (i - 2) * 0.002).astype(np.float64) for i in range(FM_NCHAN)]
    n = max(len(w) for w in waves)
    rng = np.random.default_rng(71)
    x = 1e-3 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for f, w in zip(fm_centres(), waves):
        w = np.concatenate([w, np.full(n - len(w), w[-1])])
        w = np.convolve(np.concatenate([np.full(FM_SMOOTH - 1, w[0]), w]), np.ones(FM_SMOOTH) / FM_SMOOTH, mode="valid")
        x += np.exp(2j * np.pi * np.cumsum(f + FM_DEV_HZ * w) / FM_FS) / FM_NCHAN
    x = x.astype(np.complex64)
    x.setflags(write=False)
    return x


def fm_front_end_f64(ch):
    """channel ch in float64, no block, ring or tile: convolution, every tenth sample, the angle of r[m + 1] conj(r[m])
    -> (demodulated float64[], r complex128[])"""
    x, t = fm_samples().astype(np.complex128), fm_taps()[ch].astype(np.complex128)
    m = 1 << int(np.ceil(np.log2(len(x) + len(t))))
    r = np.fft.ifft(np.fft.fft(x, m) * np.fft.fft(t, m))[:len(x)][::FM_DECI]
    return np.angle(r[1:] * np.conj(r[:-1])), r


def angle_bound(r, tol=rm.TOL):
    """the per-sample bound harness.angle_parity allows between device and oracle on the resampled stream r, computed as
    receiver_model.audio_bar computes b (gain 1)"""
    mag = np.abs(np.asarray(r).astype(np.complex128))
    eps = tol * float(mag.max())
    return tol * np.pi + eps / np.maximum(mag[:-1], 1e-30) + eps / np.maximum(mag[1:], 1e-30)


def fm_model(rows, cuts):
    """the two models over demodulated rows (one per channel) in the pushes `cuts`"""
    return chain_model(rows, cuts, FM_PRM, (1, FM_MAX_SIZE), FM_RX_KW)
