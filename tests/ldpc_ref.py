"""numpy restatement of the LDPC(648,324) mode (OFDM_ECC_LDPC648, include/ofdm_hip.h "LDPC(648,324)").  Nothing in the reference
corresponds to it (parity unpinned by the reference): this file is the definition, in exact integers, and the host functions
(ofdm_amd/csrc/ldpc_code.hip) and the kernels (k_ldpc_encode, k_ldpc_decode in ofdm_amd/csrc/kernels_ldpc.hip) are compared with it
bit for bit, iteration counts included.

The table is intended to be the n = 648, rate-1/2 matrix of 802.11n, written from memory and UNVERIFIED against the standard: the
table below is the definition.  The encoder here solves H x = 0 through a GF(2) inverse of the parity half, on purpose not the
back-substitution the library uses."""
import numpy as np

Z, ROWS, COLS = 27, 12, 24
N, M = Z * COLS, Z * ROWS                      # 648 variables, 324 checks
INFO_BYTES, CODE_BYTES = 40, 80
INFO_BITS, SENT_BITS = 8 * INFO_BYTES, 8 * CODE_BYTES
Q_MAX, R_MAX = 2047, 127
MAX_ITER = 20                                  # OFDM_LDPC_MAX_ITER: the chain's value
HEADER_STATUS, UNCORRECTABLE_STATUS = -4, -5   # OFDM_FRAME_HEADER, OFDM_FRAME_UNCORRECTABLE

_ = -1
TABLE = np.array([
    [0, _, _, _, 0, 0, _, _, 0, _, _, 0, 1, 0, _, _, _, _, _, _, _, _, _, _],
    [22, 0, _, _, 17, _, 0, 0, 12, _, _, _, _, 0, 0, _, _, _, _, _, _, _, _, _],
    [6, _, 0, _, 10, _, _, _, 24, _, 0, _, _, _, 0, 0, _, _, _, _, _, _, _, _],
    [2, _, _, 0, 20, _, _, _, 25, 0, _, _, _, _, _, 0, 0, _, _, _, _, _, _, _],
    [23, _, _, _, 3, _, _, _, 0, _, 9, 11, _, _, _, _, 0, 0, _, _, _, _, _, _],
    [24, _, 23, 1, 17, _, 3, _, 10, _, _, _, _, _, _, _, _, 0, 0, _, _, _, _, _],
    [25, _, _, _, 8, _, _, _, 7, 18, _, _, 0, _, _, _, _, _, 0, 0, _, _, _, _],
    [13, 24, _, _, 0, _, 8, _, 6, _, _, _, _, _, _, _, _, _, _, 0, 0, _, _, _],
    [7, 20, _, 16, 22, 10, _, _, 23, _, _, _, _, _, _, _, _, _, _, _, 0, 0, _, _],
    [11, _, _, _, 19, _, _, _, 13, _, 3, 17, _, _, _, _, _, _, _, _, _, 0, 0, _],
    [25, _, 8, _, 23, 18, _, 14, 9, _, _, _, _, _, _, _, _, _, _, _, _, _, 0, 0],
    [3, _, _, _, 16, _, _, 2, 25, 5, _, _, 1, _, _, _, _, _, _, _, _, _, _, 0],
], np.int64)
del _

# per block row: the variables of its 27 checks, [27, degree], edges in table order
LAYERS = []
for _l in range(ROWS):
    _cols = np.nonzero(TABLE[_l] >= 0)[0]
    LAYERS.append(np.stack([Z * c + (np.arange(Z) + TABLE[_l, c]) % Z for c in _cols], axis=1))


def parity_check_matrix() -> np.ndarray:
    """H, uint8 [324, 648]"""
    h = np.zeros((M, N), np.uint8)
    for l, var in enumerate(LAYERS):
        for z in range(Z):
            h[Z * l + z, var[z]] = 1
    return h


def gf2_rank(a) -> int:
    a = np.array(a, np.uint8) & 1
    r = 0
    for c in range(a.shape[1]):
        piv = np.nonzero(a[r:, c])[0]
        if piv.size == 0:
            continue
        a[[r, r + piv[0]]] = a[[r + piv[0], r]]
        rows = np.nonzero(a[:, c])[0]
        rows = rows[rows != r]
        a[rows] ^= a[r]
        r += 1
        if r == a.shape[0]:
            break
    return r


def gf2_inverse(a) -> np.ndarray:
    n = a.shape[0]
    w = np.concatenate([np.array(a, np.uint8) & 1, np.eye(n, dtype=np.uint8)], axis=1)
    for c in range(n):
        piv = np.nonzero(w[c:, c])[0]
        if piv.size == 0:
            raise ValueError("singular")
        w[[c, c + piv[0]]] = w[[c + piv[0], c]]
        rows = np.nonzero(w[:, c])[0]
        rows = rows[rows != c]
        w[rows] ^= w[c]
    return w[:, n:]


_ENC = None


def _encoder_matrix():
    """P [324, 324] with parity = P info' (info' = the 324 bits x[0 .. 323])"""
    global _ENC
    if _ENC is None:
        h = parity_check_matrix()
        _ENC = (gf2_inverse(h[:, M:]).astype(np.int64) @ h[:, :M].astype(np.int64)) & 1
    return _ENC


def codeword_bits(info) -> np.ndarray:
    """info uint8 [n, 40] -> x uint8 [n, 648]"""
    info = np.asarray(info, np.uint8).reshape(-1, INFO_BYTES)
    x = np.zeros((info.shape[0], N), np.uint8)
    x[:, :INFO_BITS] = np.unpackbits(info, axis=1, bitorder="little")
    x[:, M:] = (x[:, :M].astype(np.int64) @ _encoder_matrix().T) & 1
    return x


def encode(info) -> np.ndarray:
    """info uint8 [n, 40] -> code uint8 [n, 80]: x[0 .. 319] ++ x[324 .. 643], packed LSB first"""
    x = codeword_bits(info)
    return np.packbits(np.concatenate([x[:, :INFO_BITS], x[:, M:M + INFO_BITS]], axis=1), axis=1, bitorder="little")


def decode(llr, max_iter=MAX_ITER):
    """llr int8 [n, 640] (positive = bit 1) -> (bytes uint8 [n, 40], iters int32 [n]: the iteration of convergence, 0 = none)"""
    llr = np.asarray(llr, np.int64).reshape(-1, SENT_BITS)
    n = llr.shape[0]
    q = np.zeros((n, N), np.int64)
    q[:, :INFO_BITS] = -llr[:, :INFO_BITS]
    q[:, INFO_BITS:M] = Q_MAX
    q[:, M:M + INFO_BITS] = -llr[:, INFO_BITS:]
    r = [np.zeros((n,) + var.shape, np.int64) for var in LAYERS]
    iters = np.zeros(n, np.int32)
    live = np.arange(n)                      # the code words still iterating
    for it in range(1, max_iter + 1):
        if live.size == 0:
            break
        ql = q[live]
        for l, var in enumerate(LAYERS):
            t = np.clip(ql[:, var] - r[l][live], -Q_MAX, Q_MAX)              # [n, 27, deg]
            a = np.abs(t)
            order = np.sort(a, axis=2)
            m1, m2 = order[:, :, :1], order[:, :, 1:2]
            first = np.argmin(a, axis=2)[:, :, None] == np.arange(a.shape[2])  # one edge holding the minimum
            m = np.where(first, m2, m1)                                        # min over the OTHER edges
            neg = t < 0
            sign = np.where((neg.sum(axis=2, keepdims=True) - neg) & 1, -1, 1)
            rn = sign * np.minimum((3 * m) >> 2, R_MAX)
            r[l][live] = rn
            ql[:, var] = np.clip(t + rn, -Q_MAX, Q_MAX)
        q[live] = ql
        x = (ql < 0).astype(np.int64)
        ok = np.ones(live.size, bool)
        for var in LAYERS:
            ok &= ~(x[:, var].sum(axis=2) & 1).any(axis=1)
        iters[live[ok]] = it
        live = live[~ok]
    out = np.packbits((q[:, :INFO_BITS] < 0).astype(np.uint8), axis=1, bitorder="little")
    return out, iters


# ------------------------------------------------------------------------------------------------ the frame stream
def codewords(p: int) -> int:
    return (p + 8 + INFO_BYTES - 1) // INFO_BYTES


def coded_len(p: int) -> int:
    return CODE_BYTES * codewords(p)


def info_stream(payload: bytes) -> np.ndarray:
    p = len(payload)
    s = (p & 0xFFFFFFFF).to_bytes(4, "little") + ((p & 0xFFFFFFFF) ^ 0xFFFFFFFF).to_bytes(4, "little") + bytes(payload)
    s += bytes(INFO_BYTES * codewords(p) - len(s))
    return np.frombuffer(s, np.uint8)


def stream(payload: bytes) -> np.ndarray:
    """the byte stream a frame carries behind its 16-byte header"""
    return encode(info_stream(payload).reshape(-1, INFO_BYTES)).reshape(-1)


def row_bytes(body_max: int) -> int:
    """the out_stride the decode entry points ask for a body of at most body_max bytes"""
    return max(INFO_BYTES * (body_max // CODE_BYTES) - 8, 0)


def receive(llr, body: int, max_iter=MAX_ITER):
    """llr: the LLRs of the stream (LLR 0 = first bit behind the 16-byte header), `body` bytes of it demodulated.
    -> (status, bytes): (HEADER_STATUS, b"") / (UNCORRECTABLE_STATUS, b"") / (0, the delivered bytes)"""
    llr = np.asarray(llr, np.int64)
    nb = body // CODE_BYTES if body > 0 else 0
    if nb == 0:
        return HEADER_STATUS, b""
    head, it = decode(llr[:SENT_BITS], max_iter)
    hb = bytes(head[0])
    p, inv = int.from_bytes(hb[:4], "little"), int.from_bytes(hb[4:8], "little")
    if it[0] == 0 or inv != p ^ 0xFFFFFFFF:
        return HEADER_STATUS, b""
    n_cw = min(codewords(p), nb)
    out = hb
    if n_cw > 1:
        rest, its = decode(llr[SENT_BITS:n_cw * SENT_BITS].reshape(n_cw - 1, SENT_BITS), max_iter)
        if (its == 0).any():
            return UNCORRECTABLE_STATUS, b""
        out += rest.tobytes()
    return 0, out[8:8 + min(p, INFO_BYTES * nb - 8)]
