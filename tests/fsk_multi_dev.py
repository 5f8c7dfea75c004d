"""What the tests of rr.FskTxMulti share: the packet sets of the three stations, the framer's bound in Python integers, and (GPU
only; torch is imported where it is needed) one push through sentinel-filled device buffers with everything at and beyond every
stream's own counts checked on the device, as tests/fsk_dev.py does for rr.FskTx."""
import functools

import numpy as np

import frame_model as fm
import fsk_model as fk


def _packets(sizes, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in sizes]


def station_packets():
    """the packet sets of the three stations; none above 58 bytes, which is what afsk_model.MAX_SIZE = 60 lets through with the FCS"""
    return [fk.loop_packets(), _packets((40, 7), 81), _packets((33, 8, 50, 17), 80)]


@functools.lru_cache(maxsize=None)
def station_bits():
    """rr_hdlc_framer(FCS | NRZI) over each station's packets, on the CPU -> [uint8[]]"""
    return [fm.FramerSeq(fk.LOOP_FLAGS).push(ps)[0] for ps in station_packets()]


def framer_bound(packets, fcs=True):
    """rr_hdlc_framer_bound: the sum of 320 + 8 L + floor(8 L / 5), L the packet's bytes (+ 2 with the FCS)"""
    return sum(320 + 8 * L + (8 * L) // 5 for L in (len(p) + (2 if fcs else 0) for p in packets))


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
def multi_push(h, rows, counts, n_cap=None, audio=True, bits_stride=None, out_stride=None, audio_stride=None, null_counts=False):
    """one rr_fsk_tx_multi_push_dev: stream c's bits are rows[c] (at least min(counts[c], n_cap) of them; the rest of its row is
    noise) -> ([out complex64[] per stream], [audio float32[] per stream] or None, uint64[nstreams, 2] counts, launches), on the
    host.  Asserts that every element at and beyond a stream's own counts, up to the stride, still holds the sentinel."""
    import torch

    import fsk_dev as fd
    N = h.nstreams
    n_cap = max(len(r) for r in rows) if n_cap is None else n_cap
    ac, oc = h.bound(n_cap)
    bs = n_cap if bits_stride is None else bits_stride
    os_ = oc + fd.PAD if out_stride is None else out_stride
    as_ = ac + fd.PAD if audio_stride is None else audio_stride
    rng = np.random.default_rng(N * 1000 + n_cap)
    hb = rng.integers(0, 2, (N, max(bs, 1)), dtype=np.uint8)                  # noise wherever a row is not given
    for c, r in enumerate(rows):
        k = min(len(r), n_cap)
        hb[c, :k] = np.asarray(r, np.uint8)[:k]
    d_bits = torch.from_numpy(hb).cuda()
    d_cnt = None if null_counts else torch.from_numpy(np.asarray(counts, np.uint64).view(np.int64).copy()).cuda()
    d_out = torch.full((N, 2 * max(os_, 1)), fd.SENT_BITS, dtype=torch.int32, device="cuda")
    d_aud = torch.full((N, max(as_, 1)), fd.SENT_BITS, dtype=torch.int32, device="cuda") if audio else None
    torch.cuda.synchronize()
    l0 = fd.launches()
    h.push_dev(d_bits.data_ptr(), bs, n_cap, 0 if null_counts else d_cnt.data_ptr(), d_out.data_ptr(), os_,
               d_aud.data_ptr() if audio else 0, as_ if audio else 0)
    nl = fd.launches() - l0
    made = h.counts()                          # waits
    outs, auds = [], []
    for c in range(N):
        na, no = int(made[c, 0]), int(made[c, 1])
        assert na <= ac and no <= oc
        assert bool((d_out[c, 2 * no:] == fd.SENT_BITS).all()), f"stream {c}: out written at or beyond its count"
        outs.append(d_out[c, :2 * no].view(torch.float32).cpu().numpy().view(np.complex64).copy() if no else np.zeros(0, np.complex64))
        if audio:
            assert bool((d_aud[c, na:] == fd.SENT_BITS).all()), f"stream {c}: audio written at or beyond its count"
            auds.append(d_aud[c, :na].view(torch.float32).cpu().numpy().copy())
    return outs, (auds if audio else None), made, nl
