"""The captures the EXT-5 tests share (tests/test_chest_cpu.py, tests/test_gpu_chest.py): six 64-QAM frames with guard bands through
the oracle's channel, payload bytes from default_rng(3), channel seeds 100 .. 105 -- N = 1024 / payload 1304 / 28 dB and N = 64 /
payload 560 / 14 dB.  Everything here is the f64 oracle and numpy; results are cached per (n_fft, snr)."""
import functools

import numpy as np

QAM64 = 6
FRAMES = 6
SEED0 = 100
PAYLOAD = {64: 560, 1024: 1304}
WORTH = ((1024, 28.0), (64, 14.0))          # (n_fft, snr_db) of the "worth" table


def payloads(n_fft):
    return np.random.default_rng(3).integers(0, 256, (FRAMES, PAYLOAD[n_fft]), dtype=np.uint8)


def bits(b):
    return np.unpackbits(np.frombuffer(bytes(b), np.uint8))


@functools.lru_cache(maxsize=None)
def captures(n_fft, snr_db):
    """-> list of dicts per frame: tx, rx (noisy capture), clean (the same frame, same channel, 300 dB), offset (the oracle's
    Schmidl-Cox start), h_ls / h_clean (the oracle's estimate_channel of the noisy / the clean capture at that offset), n_sym (data
    symbols), ref_bits (hard bits of the clean capture demodulated with h_clean, over the 16 + payload bytes the frame carries)"""
    from oracle import oracle as orc

    S = n_fft + n_fft // 4
    trn = orc.default_training(n_fft)
    out = []
    for i, pay in enumerate(payloads(n_fft)):
        tx = orc.encode(bytes(pay), guard=True, modulation=QAM64, n_fft=n_fft)
        rx, _ = orc.channel(tx, snr_db, False, SEED0 + i)
        clean, _ = orc.channel(tx, 300.0, False, SEED0 + i)
        off = orc.decode_sc(rx, guard=True, modulation=QAM64, n_fft=n_fft)["offset"]
        n_sym = len(tx) // S - 10
        h_ls = orc.estimate_channel(rx[off + 5 * S:off + 10 * S], trn, n_fft)
        h_clean = orc.estimate_channel(clean[off + 5 * S:off + 10 * S], trn, n_fft)
        c = dict(tx=tx, rx=rx, clean=clean, offset=off, n_sym=n_sym, h_ls=h_ls, h_clean=h_clean, n_bytes=16 + pay.size)
        c["ref_bits"] = bits(orc.rx_demod(clean[off + 10 * S:off + (10 + n_sym) * S], n_fft, True, QAM64, hk=h_clean)[:c["n_bytes"]])
        out.append(c)
    return out


def hard_errors(n_fft, cap, hk):
    """bit errors of the noisy capture demodulated with hk, against the noiseless demodulation of the same frame"""
    from oracle import oracle as orc

    S = n_fft + n_fft // 4
    off = cap["offset"]
    got = orc.rx_demod(cap["rx"][off + 10 * S:off + (10 + cap["n_sym"]) * S], n_fft, True, QAM64, hk=hk)[:cap["n_bytes"]]
    return int((bits(got) != cap["ref_bits"]).sum())
