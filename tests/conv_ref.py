"""numpy restatement of the K = 7 rate-1/2 convolutional code (OFDM_ECC_CONV_K7, include/ofdm_hip.h "convolutional code"): the
encoder with generators 133 / 171 (octal) and one zero tail byte, and the exact soft-input Viterbi decoder on integer LLRs.  The
counterpart of tests/soft_ref.py: the GPU kernels (ofdm_amd/csrc/kernels_conv.hip) are compared with this bit for bit."""
import itertools

import numpy as np

G0, G1 = 0o133, 0o171
PAR = np.array([bin(i).count("1") & 1 for i in range(128)], np.int64)


def encode_bits(u) -> np.ndarray:
    """input bits u_t -> coded bits c_{2t} = A_t, c_{2t+1} = B_t, from state 0 (no tail is added here)"""
    s, c = 0, []
    for b in np.asarray(u, np.int64):
        r = (int(b) << 6) | s
        c += [PAR[r & G0], PAR[r & G1]]
        s = r >> 1
    return np.array(c, np.uint8)


def encode(payload: bytes) -> np.ndarray:
    """payload bytes + one 0x00 tail byte, LSB first -> 2 (p + 1) coded bytes, packed LSB first"""
    u = np.unpackbits(np.frombuffer(bytes(payload) + b"\0", np.uint8), bitorder="little")
    return np.packbits(encode_bits(u), bitorder="little")


_SP = np.arange(64)
_U, _P0 = _SP >> 5, (_SP & 31) << 1
_P1 = _P0 | 1
_R0, _R1 = (_U << 6) | _P0, (_U << 6) | _P1
_SA0, _SB0 = 2 * PAR[_R0 & G0] - 1, 2 * PAR[_R0 & G1] - 1
_SA1, _SB1 = 2 * PAR[_R1 & G0] - 1, 2 * PAR[_R1 & G1] - 1


def viterbi(llr, terminated=True) -> np.ndarray:
    """2 T LLRs (positive = bit 1) -> T // 8 bytes.  Metrics are maximised; a tie keeps predecessor p0; the traceback starts at
    state 0 (terminated) or at the first = lowest state of the largest final metric."""
    llr = np.asarray(llr, np.int64)
    T = llr.size // 2
    pm = np.full(64, -(1 << 40), np.int64)
    pm[0] = 0
    dec = np.zeros((T, 64), np.uint8)
    for t in range(T):
        la, lb = llr[2 * t], llr[2 * t + 1]
        c0 = pm[_P0] + _SA0 * la + _SB0 * lb
        c1 = pm[_P1] + _SA1 * la + _SB1 * lb
        d = c1 > c0
        dec[t] = d
        pm = np.where(d, c1, c0)
    s = 0 if terminated else int(np.argmax(pm))
    bits = np.zeros(T, np.uint8)
    for t in range(T - 1, -1, -1):
        bits[t] = s >> 5
        s = ((s & 31) << 1) | int(dec[t, s])
    return np.packbits(bits[: T // 8 * 8], bitorder="little")


def viterbi_batch(llr, terminated=True) -> np.ndarray:
    """viterbi() for every row of llr [F, 2 T] at once -> [F, T // 8]: the same recursion with a frame axis (the tests check it
    against viterbi())."""
    llr = np.asarray(llr, np.int64)
    F, T = llr.shape[0], llr.shape[1] // 2
    pm = np.full((F, 64), -(1 << 40), np.int64)
    pm[:, 0] = 0
    dec = np.zeros((T, F, 64), np.uint8)
    for t in range(T):
        la, lb = llr[:, 2 * t, None], llr[:, 2 * t + 1, None]
        c0 = pm[:, _P0] + _SA0 * la + _SB0 * lb
        c1 = pm[:, _P1] + _SA1 * la + _SB1 * lb
        d = c1 > c0
        dec[t] = d
        pm = np.where(d, c1, c0)
    s = np.zeros(F, np.int64) if terminated else np.argmax(pm, axis=1)
    bits = np.zeros((F, T), np.uint8)
    rows = np.arange(F)
    for t in range(T - 1, -1, -1):
        bits[:, t] = s >> 5
        s = ((s & 31) << 1) | dec[t, rows, s]
    if T // 8 == 0:
        return np.zeros((F, 0), np.uint8)
    return np.packbits(bits[:, : T // 8 * 8], axis=1, bitorder="little")


def brute_force(llr, terminated=True):
    """(best input bits, whether the maximum is unique) over ALL T-bit inputs (terminated: those whose last six bits are zero)"""
    llr = np.asarray(llr, np.int64)
    T = llr.size // 2
    free = T - 6 if terminated else T
    best, best_u, unique = None, None, True
    for tup in itertools.product((0, 1), repeat=free):
        u = np.array(tup + (0,) * (T - free), np.int64)
        m = int(((2 * encode_bits(u).astype(np.int64) - 1) * llr[: 2 * T]).sum())
        if best is None or m > best:
            best, best_u, unique = m, u, True
        elif m == best:
            unique = False
    return best_u.astype(np.uint8), unique
