"""Vectors and the host reference for the batched RS(255,223) tests (tests/test_rs_modes_cpu.py, tests/test_gpu_rs.py).

The definition the device is held to is the host decoder ofdm_rs255_decode, block by block; test_rs_modes_cpu.py pins that decoder
to the oracle's decipher_transmission_bytes on exactly these vectors."""
import ctypes as C

import numpy as np

N, K = 255, 223
ROWS = 7
N_CODES = (0, 1, 254, 255, 256, 765, 766, 1020)
# what is done to block b of row r: KINDS[(r + 7 b) % 10] -- one block a row covers the first seven, three blocks a row all of them
KINDS = ("clean", "e1", "e16", "e17", "random", "forced", "parity", "e2", "e15", "zero")


def host_encode(lib, data: bytes) -> bytes:
    src = np.frombuffer(bytes(data), np.uint8).copy()
    out = np.zeros(N * (src.size // K + 1), np.uint8)
    assert lib.ofdm_rs255_encode(C.c_void_p(src.ctypes.data) if src.size else None, C.c_int64(src.size), C.c_void_p(out.ctypes.data)) == 0
    return bytes(out)


def host_block(lib, block: np.ndarray):
    """(223 bytes, corrected) of one zero-padded 255-byte block by the host decoder; corrected = -1 and the received data bytes
    where it reports OFDM_ERR_UNCORRECTABLE"""
    blk = np.ascontiguousarray(block, np.uint8)
    assert blk.size == N
    out = np.zeros(2 * K, np.uint8)                       # the block and the empty remainder behind it
    fixed = C.c_int32(0)
    rc = lib.ofdm_rs255_decode(C.c_void_p(blk.ctypes.data), C.c_int64(N), C.c_void_p(out.ctypes.data), C.byref(fixed))
    if rc == -6:
        return bytes(blk[:K]), -1
    assert rc == 0
    return bytes(out[:K]), int(fixed.value)


def host_row(lib, row: np.ndarray, length: int):
    """(bytes, out_len, corrected) of the first `length` bytes of a row, as ofdm_rs255_decode_batch defines it"""
    code = np.asarray(row, np.uint8)[:length]
    blocks = length // N + 1
    padded = np.zeros(blocks * N, np.uint8)
    padded[:length] = code
    out, total, bad = b"", 0, False
    for b in range(blocks):
        data, fixed = host_block(lib, padded[b * N:(b + 1) * N])
        out += data
        bad = bad or fixed < 0
        total += max(fixed, 0)
    return out, K * blocks, (-1 if bad else total)


def decoder_rows(lib, n_code: int, seed: int = 2255) -> np.ndarray:
    """ROWS rows of n_code code bytes: code words of random data, every whole block treated by its KIND; the bytes of a cut last block
    are the head of a code word"""
    rng = np.random.default_rng(seed + n_code)
    blocks = n_code // N + 1
    rows = np.zeros((ROWS, blocks * N), np.uint8)
    for r in range(ROWS):
        data = rng.integers(0, 256, blocks * K - 1, dtype=np.uint8)       # (blocks * 223 - 1) // 223 + 1 = blocks
        rows[r] = np.frombuffer(host_encode(lib, bytes(data)), np.uint8)
        for b in range(n_code // N):                                      # whole blocks only
            kind = KINDS[(r + ROWS * b) % len(KINDS)]
            blk = rows[r, b * N:(b + 1) * N]
            if kind.startswith("e"):
                pos = rng.choice(N, int(kind[1:]), replace=False)
                blk[pos] ^= rng.integers(1, 256, pos.size, dtype=np.uint8)
            elif kind == "random":
                blk[:] = rng.integers(0, 256, N, dtype=np.uint8)
            elif kind == "forced":
                blk[[0, 222, 223, 254]] ^= rng.integers(1, 256, 4, dtype=np.uint8)
            elif kind == "parity":
                pos = K + rng.choice(N - K, 5, replace=False)
                blk[pos] ^= rng.integers(1, 256, 5, dtype=np.uint8)
            elif kind == "zero":
                blk[:] = 0
    return np.ascontiguousarray(rows[:, :n_code])


def row_lengths(n_code: int) -> np.ndarray:
    """per-row code_len: the whole row, 0, lengths that cut a block, and two values outside [0, n_code] (clamped)"""
    return np.array([n_code, 0, n_code - 1, min(N, n_code), min(100, n_code), n_code + 7, -3], np.int32)


def clamp(length: int, n_code: int) -> int:
    return min(max(int(length), 0), n_code)
