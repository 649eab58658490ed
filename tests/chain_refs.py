"""What the decode chains must deliver, composed from the stage entry points and the CPU restatements -- shared by the tests of the
modes (tests/test_gpu_soft.py, test_gpu_conv.py, test_gpu_rs.py) and by tests/test_gpu_forged_header.py.  Every helper reads the
16-byte length header from the hard bytes rx_demod returns for the chain's own offset / f_delta / channel estimate and applies the
rule of src/receiver.rs:85-95 in plain integers."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_ref as cr  # noqa: E402
import rs_vectors as rv  # noqa: E402
import soft_ref as sr  # noqa: E402

UNCORRECTABLE = -5


def hard_and_llrs(c, rx, r, max_symbols, want_llr=True):
    """(hard bytes [F, max_symbols * bytes_per_symbol], LLRs [F, 8 times as many] or None) of the data symbols, demodulated with the
    chain's own timing, CFO and channel estimate"""
    hk = c.estimate_channel(rx, r["offset"], r["f_delta"])
    L = c.rx_llr(rx, max_symbols, first_symbol=10, offset=r["offset"], f_delta=r["f_delta"], hk=hk) if want_llr else None
    hard = c.rx_demod(rx, max_symbols, first_symbol=10, offset=r["offset"], f_delta=r["f_delta"], hk=hk)
    c.synchronize()
    return hard.cpu().numpy(), (None if L is None else L.cpu().numpy())


def header_of(hard_row):
    """(lo, hi) of the little-endian u128 a row of hard bytes starts with"""
    return int.from_bytes(bytes(hard_row[:8]), "little"), int.from_bytes(bytes(hard_row[8:16]), "little")


def soft_reference_decode(c, rx, r, max_symbols):
    """OFDM_ECC_HAMMING74_SOFT, per frame with status 0: (out_len, bytes) -- the length header from the hard bytes, then
    soft_ref.ham_decode_soft over the floor(keep / 7) blocks of the LLRs rx_llr returns for the frame, from LLR 128 on"""
    hard, L = hard_and_llrs(c, rx, r, max_symbols)
    body = max_symbols * c.bytes_per_symbol - 16
    want = {}
    for f in range(rx.shape[0]):
        if int(r["status"][f]) != 0:
            continue
        lo, hi = header_of(hard[f])
        keep = lo if (hi == 0 and lo < body) else body
        blocks = keep // 7
        want[f] = (4 * blocks, bytes(sr.ham_decode_soft(L[f, 128:128 + 56 * blocks])))
    return want


def conv_reference_decode(c, rx, r, max_symbols):
    """OFDM_ECC_CONV_K7, per frame with status 0: (out_len, bytes) by the rule of the header -- the length header from the hard bytes,
    then conv_ref.viterbi over the LLRs rx_llr returns for the frame"""
    hard, L = hard_and_llrs(c, rx, r, max_symbols)
    body = max_symbols * c.bytes_per_symbol - 16
    want = {}
    for f in range(rx.shape[0]):
        if int(r["status"][f]) != 0:
            continue
        lo, hi = header_of(hard[f])
        keep = lo if (hi == 0 and lo < body) else body
        n_out = max(keep // 2 - 1, 0)
        dec = cr.viterbi(L[f, 128:128 + 8 * keep], terminated=(hi == 0 and lo <= body))
        want[f] = (n_out, bytes(dec[:n_out]))
    return want


def rs_composition(c, rx, max_symbols):
    """OFDM_ECC_RS255*: what the RS mode must deliver -- the host RS decoder over what the inner mode's context delivers for the same
    capture.  -> (the inner mode's result, [(status, out_len, bytes)] per frame)"""
    from ofdm_amd import api

    inner = api.Context(n_fft=c.n_fft, modulation=c.modulation, guard_bands=c.guard_bands, ecc=c.ecc - 20)
    ri = inner.decode_batch(rx, max_symbols=max_symbols)
    inner.synchronize()
    status, ln, by = ri["status"].cpu().numpy(), ri["len"].cpu().numpy(), ri["bytes"].cpu().numpy()
    want = []
    for f in range(rx.shape[0]):
        if status[f] != 0:
            want.append((int(status[f]), 0, b""))
            continue
        data, out_len, fixed = rv.host_row(c.lib, by[f], int(ln[f]))
        want.append((UNCORRECTABLE, 0, b"") if fixed < 0 else (0, out_len, data))
    return ri, want
