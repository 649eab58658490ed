"""The LLR sets tests/test_ldpc_cpu.py decodes with the host decoder and tests/test_gpu_ldpc.py decodes on the device, and their
decode by tests/ldpc_ref.py, computed once per (set, max_iter) and shared."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ldpc_ref as lr  # noqa: E402

NOISY_CODEWORDS = 420
NOISY_EBN0_DB = 1.5          # BPSK over AWGN, LLR = clamp(rint(32 y), +-127): ldpc_ref leaves a fifth to a quarter unconverged at 20 iterations
MAX_ITERS = (1, 5, 20, 64)


@functools.lru_cache(maxsize=None)
def noisy():
    """-> (info uint8 [n, 40], llr int8 [n, 640])"""
    rng = np.random.default_rng(648324)
    info = rng.integers(0, 256, (NOISY_CODEWORDS, lr.INFO_BYTES), dtype=np.uint8)
    bits = np.unpackbits(lr.encode(info), axis=1, bitorder="little").astype(np.float64)
    sigma = np.sqrt(1.0 / (2.0 * 0.5 * 10.0 ** (NOISY_EBN0_DB / 10.0)))    # rate 1/2
    y = (2.0 * bits - 1.0) + sigma * rng.standard_normal(bits.shape)
    return info, np.clip(np.rint(32.0 * y), -127, 127).astype(np.int8)


@functools.lru_cache(maxsize=None)
def clean():
    """-> (info uint8 [24, 40], llr int8 [24, 640]): noiseless +-32"""
    rng = np.random.default_rng(27)
    info = rng.integers(0, 256, (24, lr.INFO_BYTES), dtype=np.uint8)
    bits = np.unpackbits(lr.encode(info), axis=1, bitorder="little").astype(np.int64)
    return info, (32 * (2 * bits - 1)).astype(np.int8)


@functools.lru_cache(maxsize=None)
def corner():
    """all-zero, all -128, all +127 and uniformly random int8 rows"""
    rng = np.random.default_rng(324)
    rows = [np.zeros((1, lr.SENT_BITS), np.int8), np.full((1, lr.SENT_BITS), -128, np.int8), np.full((1, lr.SENT_BITS), 127, np.int8),
            rng.integers(-128, 128, (9, lr.SENT_BITS), dtype=np.int8)]
    return np.concatenate(rows)


def llr_set(name):
    return {"clean": lambda: clean()[1], "corner": corner, "noisy": lambda: noisy()[1]}[name]()


@functools.lru_cache(maxsize=None)
def reference(name, max_iter):
    """ldpc_ref.decode of a set -> (bytes [n, 40], iters [n])"""
    return lr.decode(llr_set(name), max_iter)


@functools.lru_cache(maxsize=None)
def mixed(n, max_iter=lr.MAX_ITER):
    """n code words drawn from all three sets in a fixed shuffled order -> (llr [n, 640], bytes [n, 40], iters [n]) with the reference's
    decode of each"""
    parts = [(llr_set(s),) + reference(s, max_iter) for s in ("clean", "corner", "noisy")]
    llr, by, it = (np.concatenate([p[i] for p in parts]) for i in range(3))
    pick = np.random.default_rng(n).permutation(llr.shape[0])
    pick = np.resize(pick, n)
    return llr[pick], by[pick], it[pick]
