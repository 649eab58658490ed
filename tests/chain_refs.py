"""What the decode chains must deliver, composed from the stage entry points and the CPU restatements -- shared by the tests of the
modes (tests/test_gpu_soft.py, test_gpu_conv.py, test_gpu_rs.py) and by tests/test_gpu_forged_header.py; the assertions those tests
share are tests/chain_checks.py, the seeded link they run over is tools/link.py.  Every decode helper reads the
16-byte length header from the hard bytes rx_demod returns for the chain's own offset / f_delta / channel estimate and applies the
rule of src/receiver.rs:85-95 in plain integers."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_ref as cr  # noqa: E402
import fcs_ref  # noqa: E402
import framed_ref as fr  # noqa: E402
import ldpc_rates_ref as lrr  # noqa: E402
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


def decoder_rows(rng, n_steps, per_kind):
    """LLR rows [4 * per_kind, 2 n_steps]: noisy codewords, uniform int8, all zero, +-127 along one codeword; and the bytes behind
    the last kind"""
    u = rng.integers(0, 2, (2 * per_kind, n_steps))
    u[:, max(n_steps - 8, 0):] = 0                               # (a zero tail where there is room for one; not required)
    code = np.stack([cr.encode_bits(r) for r in u]).astype(np.int64).reshape(2 * per_kind, 2 * n_steps)
    noisy = np.clip(np.rint((2 * code[:per_kind] - 1) * 20 + rng.normal(0, 22, (per_kind, 2 * n_steps))), -127, 127)
    uniform = rng.integers(-128, 128, (per_kind, 2 * n_steps))
    zero = np.zeros((per_kind, 2 * n_steps), np.int64)
    hard = (2 * code[per_kind:] - 1) * 127                        # the largest metrics a frame can produce
    sent = np.packbits(u[per_kind:, : n_steps // 8 * 8], axis=1, bitorder="little") if n_steps >= 8 else np.zeros((per_kind, 0), np.uint8)
    return np.concatenate([noisy, uniform, zero, hard]).astype(np.int8), sent


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


# ---- a mode as a whole (tests/test_gpu_modes.py): ecc = [64 +] [20 +] inner, the lengths composed layer by layer from the references
# every ecc value ofdm_create takes (tests/test_gpu_modes.py holds the list to the library); fcs_ref.BASE_MODES is the same list
BASE_MODES = (0, 1, 2, 5, 10, 11, 12, 16, 20, 30, 31, 32, 41, 42, 43)
ALL_MODES = BASE_MODES + tuple(fcs_ref.ECC_FCS + m for m in BASE_MODES)
assert fcs_ref.BASE_MODES == BASE_MODES and len(ALL_MODES) == 30


def mode_layers(ecc):
    """(frame check?, RS outer code?, inner mode)"""
    fcs = ecc >= fcs_ref.ECC_FCS
    base = ecc - fcs_ref.ECC_FCS if fcs else ecc
    rs = base in (20, 30, 31, 32)
    return fcs, rs, base - 20 if rs else base


def mode_coded_len(ecc, p):
    """bytes a frame of mode ecc carries behind its 16-byte header for a payload of p bytes"""
    fcs, rs, inner = mode_layers(ecc)
    if fcs:
        p += fcs_ref.OVERHEAD
    if rs:
        p = 255 * (p // 223 + 1)                 # whole blocks and the trailing zero block
    if inner == 0:
        return p
    if inner in (1, 2):
        return 7 * -(-p // 4)
    if inner == 5:
        return 2 * (p + 1)
    return lrr.code_of_ecc(inner).coded_len(p) if inner in lrr.ECC else fr.coded_len(p, inner - 10)


def mode_row_bytes(ecc, body):
    """the largest row the decode chain of mode ecc can deliver for a demodulated body of `body` bytes: the out_stride it asks for"""
    fcs, rs, inner = mode_layers(ecc)
    if inner == 0:
        row = body
    elif inner in (1, 2):
        row = 4 * (body // 7)
    elif inner == 5:
        row = max(body // 2 - 1, 0)
    elif inner in lrr.ECC:
        row = lrr.code_of_ecc(inner).row_bytes(body)
    else:
        row = fr.max_steps(8 * (body - fr.LENGTH_BLOCK), inner - 10) // 8 if body >= fr.LENGTH_BLOCK else 0
    if rs:
        row = 223 * (row // 255 + 1)
    return max(row - fcs_ref.OVERHEAD, 0) if fcs else row
