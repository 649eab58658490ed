"""The LLR sets tests/test_ldpc_rates_cpu.py decodes with the host decoder and tests/test_gpu_ldpc_rates.py decodes on the device, and
their decode by tests/ldpc_rates_ref.py, computed once per (rate, max_iter) and shared."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ldpc_rates_ref as rr  # noqa: E402

MAX_ITERS = (1, 20)
# BPSK over AWGN, LLR = clamp(rint(32 y), +-127), Eb/N0 in dB with the rate taken as 8 K / 640: below the code's waterfall (most words
# never converge), inside it (late convergence) and far above it (the first iteration's checks hold)
NOISY_EBN0_DB = ((0.75, 2.0, 8.0), (1.25, 2.75, 8.0), (1.75, 3.25, 8.0), (2.75, 4.25, 9.0))
NOISY_PER_LEVEL = 14


def awgn_llr(code, info, ebn0_db, rng):
    """info uint8 [n, K] through the code's real shortening and puncturing -> llr int8 [n, 640]"""
    bits = np.unpackbits(code.encode(info), axis=1, bitorder="little").astype(np.float64)
    rate = code.info_bits / rr.SENT_BITS
    sigma = np.sqrt(1.0 / (2.0 * rate * 10.0 ** (ebn0_db / 10.0)))
    y = (2.0 * bits - 1.0) + sigma * rng.standard_normal(bits.shape)
    return np.clip(np.rint(32.0 * y), -127, 127).astype(np.int8)


@functools.lru_cache(maxsize=None)
def pool(rate):
    """-> (llr int8 [n, 640], info uint8 [n, K] (zeros where no code word was sent), kind [n]): 'clean' (noiseless +-32), 'junk'
    (uniformly random int8), 'zero', 'low' (-128), 'high' (+127) and 'noisy<level>' rows.  The order is part of the definition: rows 0 ..
    3 are clean, junk, junk, clean and rows 6, 7 junk, clean, so that in rows of two and of three code words a word that converges at
    once sits side by side on the device with one that never does, on either half."""
    code = rr.CODES[rate]
    rng = np.random.default_rng(6480 + rate)
    llr, info, kind = [], [], []

    def add(l, i, k):
        llr.append(np.asarray(l, np.int8).reshape(rr.SENT_BITS)); info.append(i); kind.append(k)

    none = np.zeros(code.k, np.uint8)
    clean_info = rng.integers(0, 256, (6, code.k), dtype=np.uint8)
    clean = (32 * (2 * np.unpackbits(code.encode(clean_info), axis=1, bitorder="little").astype(np.int64) - 1)).astype(np.int8)
    junk = rng.integers(-128, 128, (6, rr.SENT_BITS), dtype=np.int8)
    add(clean[0], clean_info[0], "clean")
    add(junk[0], none, "junk")
    add(junk[1], none, "junk")
    add(clean[1], clean_info[1], "clean")
    add(np.zeros(rr.SENT_BITS), none, "zero")
    add(np.full(rr.SENT_BITS, -128), none, "low")
    add(junk[2], none, "junk")
    add(clean[2], clean_info[2], "clean")
    add(np.full(rr.SENT_BITS, 127), none, "high")
    for level, db in enumerate(NOISY_EBN0_DB[rate]):
        ni = rng.integers(0, 256, (NOISY_PER_LEVEL, code.k), dtype=np.uint8)
        for l, i in zip(awgn_llr(code, ni, db, rng), ni):
            add(l, i, f"noisy{level}")
    for j in range(3, 6):
        add(clean[j], clean_info[j], "clean")
        add(junk[j], none, "junk")
    return np.stack(llr), np.stack(info), tuple(kind)


@functools.lru_cache(maxsize=None)
def reference(rate, max_iter):
    """ldpc_rates_ref's decode of the pool -> (bytes [n, K], iters [n])"""
    return rr.CODES[rate].decode(pool(rate)[0], max_iter)


def rows(rate, n_rows, n_cw, max_iter):
    """n_rows rows of n_cw code words taken from the pool in its order (wrapping) -> (llr [n_rows, n_cw * 640], bytes [n_rows * n_cw, K],
    iters [n_rows * n_cw])"""
    llr = pool(rate)[0]
    by, it = reference(rate, max_iter)
    pick = np.resize(np.arange(llr.shape[0]), n_rows * n_cw)
    return llr[pick].reshape(n_rows, n_cw * rr.SENT_BITS), by[pick], it[pick]
