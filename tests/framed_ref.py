"""numpy restatement of the punctured rates and the framed convolutional modes (OFDM_ECC_CONV_K7F_R12 / _R23 / _R34, include/ofdm_hip.h
"punctured rates and framed modes"), built on tests/conv_ref.py.  Nothing in the reference corresponds to these modes (parity
unpinned by the reference): this file is the definition, and the GPU kernels (k_conv_encode_p, k_viterbi_k7f in
ofdm_amd/csrc/kernels_conv.hip) are compared with it bit for bit."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_ref as cr  # noqa: E402

RATE_1_2, RATE_2_3, RATE_3_4 = 0, 1, 2
RATES = (RATE_1_2, RATE_2_3, RATE_3_4)
# keep mask per rate, periodic in the step index t: (A_t, B_t) -- the 802.11a patterns
MASKS = {RATE_1_2: ((1, 1),), RATE_2_3: ((1, 1), (1, 0)), RATE_3_4: ((1, 1), (1, 0), (0, 1))}
LENGTH_BLOCK = 18            # bytes: the rate-1/2 code of [u32 LE p][u32 LE ~p] and the tail byte, 72 steps
HEADER_STATUS = -4           # OFDM_FRAME_HEADER


def keep_mask(T: int, rate: int) -> np.ndarray:
    """bool [2 T]: whether coded bit c_j of steps 0 .. T - 1 is kept"""
    m = np.array(MASKS[rate], bool)
    return m[np.arange(T) % len(m)].reshape(-1)


def kept(T: int, rate: int) -> int:
    """the number of ones in the mask over steps 0 .. T - 1: whole periods, then the ones of the started period"""
    m = MASKS[rate]
    return (T // len(m)) * sum(a + b for a, b in m) + sum(a + b for a, b in m[: T % len(m)])


def max_steps(bits: int, rate: int) -> int:
    """the largest T with kept(T, rate) <= bits"""
    if bits <= 0:
        return 0
    upto = keep_mask(bits, rate).reshape(-1, 2).sum(axis=1).cumsum()      # kept(t + 1, rate) for t in [0, bits); kept(T) >= T
    return int((upto <= bits).sum())


def puncture(coded_bits, rate: int) -> np.ndarray:
    """the kept bits of c_0, c_1, ... in order"""
    c = np.asarray(coded_bits)
    return c[keep_mask(c.size // 2, rate)]


def depuncture(llr, T: int, rate: int) -> np.ndarray:
    """kept(T, rate) LLRs -> 2 T LLRs with 0 at every dropped position"""
    full = np.zeros(2 * T, np.int64)
    full[keep_mask(T, rate)] = np.asarray(llr, np.int64)[: kept(T, rate)]
    return full


def body_len(p: int, rate: int) -> int:
    return (kept(8 * (p + 1), rate) + 7) // 8


def coded_len(p: int, rate: int) -> int:
    return LENGTH_BLOCK + body_len(p, rate)


def encode_punctured(payload: bytes, rate: int) -> np.ndarray:
    """payload + tail byte at `rate`: the punctured stream packed LSB first, zero-padded to a whole byte"""
    bits = np.unpackbits(cr.encode(payload), bitorder="little")
    return np.packbits(puncture(bits, rate), bitorder="little")


def length_block(p: int) -> np.ndarray:
    p &= 0xFFFFFFFF
    return cr.encode(p.to_bytes(4, "little") + (p ^ 0xFFFFFFFF).to_bytes(4, "little"))


def encode_stream(payload: bytes, rate: int) -> np.ndarray:
    """the byte stream a framed frame carries behind its 16-byte header: [length block][body]"""
    return np.concatenate([length_block(len(payload)), encode_punctured(payload, rate)])


def length_block_value(block9):
    """the 9 decoded bytes of a length block -> p, or None when the block is invalid"""
    b = bytes(block9)
    lo, hi = int.from_bytes(b[:4], "little"), int.from_bytes(b[4:8], "little")
    return lo if (hi == lo ^ 0xFFFFFFFF and b[8] == 0) else None


def viterbi_punctured(llr, T: int, rate: int, terminated=True) -> np.ndarray:
    return cr.viterbi(depuncture(llr, T, rate), terminated)


def decode_stream(llr, avail_bytes: int, rate: int):
    """llr: the LLRs of the stream (LLR 0 = first bit behind the 16-byte header), avail_bytes of it demodulated.
    -> (status, bytes): (HEADER_STATUS, b"") without a valid length, else (0, the delivered bytes)"""
    llr = np.asarray(llr, np.int64)
    if avail_bytes < LENGTH_BLOCK:
        return HEADER_STATUS, b""
    p = length_block_value(cr.viterbi(llr[: 8 * LENGTH_BLOCK], True))
    if p is None:
        return HEADER_STATUS, b""
    avail = avail_bytes - LENGTH_BLOCK
    body = llr[8 * LENGTH_BLOCK:]
    if body_len(p, rate) <= avail:
        return 0, bytes(viterbi_punctured(body, 8 * (p + 1), rate, True)[:p])
    T = max_steps(8 * avail, rate)
    return 0, bytes(viterbi_punctured(body, T, rate, False)[: min(p, T // 8)])
