"""numpy restatement of the LDPC(648) family (OFDM_ECC_LDPC648 / _R23 / _R34 / _R56, include/ofdm_hip.h "LDPC(648), rates 2/3, 3/4 and
5/6").  Nothing in the reference corresponds to it (parity unpinned by the reference): this file is the definition, in exact integers,
and the host functions (ofdm_ldpc648_*_rate in ofdm_amd/csrc/ldpc_code.hip) and the kernels (k_ldpc_encode<r..>, k_ldpc_decode<r..>
in ofdm_amd/csrc/kernels_ldpc.hip) are compared with it bit for bit, iteration counts included.

It generalises tests/ldpc_ref.py by the table and the sent map; for rate 0 it is that file again (tests/test_ldpc_rates_cpu.py holds
the two together).  The tables of rates 2/3, 3/4 and 5/6 are the project's own, found by a seeded greedy search (row degrees balanced,
no 4-cycles, the fewest 6-cycles of 30 draws): they are NOT the matrices of 802.11n, and the tables below are the definition.  The
encoder here solves H x = 0 through a GF(2) inverse of the parity half, on purpose not the back-substitution the library uses."""
import functools

import numpy as np

import ldpc_ref as lr

Z, COLS, N = 27, 24, 648
CODE_BYTES, SENT_BITS = 80, 640
Q_MAX, R_MAX = 2047, 127
MAX_ITER = 20                                  # OFDM_LDPC_MAX_ITER: the chain's value
HEADER_STATUS, UNCORRECTABLE_STATUS = -4, -5   # OFDM_FRAME_HEADER, OFDM_FRAME_UNCORRECTABLE
RATES = (0, 1, 2, 3)                           # 1/2, 2/3, 3/4, 5/6
INFO_BYTES = (40, 53, 60, 67)                  # K
ECC = (16, 41, 42, 43)                         # OFDM_ECC_LDPC648, _R23, _R34, _R56

_ = -1
TABLES = (
    lr.TABLE,
    np.array([
        [15, 5, 24, _, 3, 14, _, _, 8, 23, _, 4, _, _, 13, _, 1, 0, _, _, _, _, _, _],
        [5, 2, 12, 9, _, 17, _, 1, _, _, 10, _, 26, _, _, _, _, 0, 0, _, _, _, _, _],
        [21, 24, 22, 2, _, 2, 25, _, 4, _, _, 5, _, _, _, _, _, _, 0, 0, _, _, _, _],
        [26, 13, 7, 22, _, _, 15, _, 11, _, 18, _, 17, _, _, 4, _, _, _, 0, 0, _, _, _],
        [0, 5, _, 15, 0, 24, _, 11, _, 10, _, _, _, 0, 1, _, 0, _, _, _, 0, 0, _, _],
        [3, 21, 18, 12, 22, _, 25, _, _, 22, _, _, 16, _, _, 5, _, _, _, _, _, 0, 0, _],
        [5, 14, 22, 8, _, _, 13, 14, _, _, 18, _, _, 2, _, 11, _, _, _, _, _, _, 0, 0],
        [4, 17, 7, 5, 26, _, _, 3, _, _, _, 5, _, 8, 16, _, 1, _, _, _, _, _, _, 0],
    ], np.int64),
    np.array([
        [11, 13, 17, 14, 16, _, 14, 20, _, 26, _, 2, 26, _, _, 26, 23, _, 1, 0, _, _, _, _],
        [21, 3, 11, 15, 13, 26, 5, _, _, 15, _, 8, _, 13, _, 21, _, 18, _, 0, 0, _, _, _],
        [22, 1, 21, 6, 21, 8, _, 20, 25, _, 16, _, 9, _, _, 17, _, 25, _, _, 0, 0, _, _],
        [18, 22, 11, 25, 18, 13, _, 13, 26, _, 22, _, 21, _, 16, _, 4, _, 0, _, _, 0, 0, _],
        [13, 18, 5, 12, 20, _, 3, 21, 0, _, _, 11, _, 25, 8, _, 19, _, _, _, _, _, 0, 0],
        [25, 22, 21, 3, 13, 24, 10, _, _, 24, 12, _, _, 3, 10, _, _, 3, 1, _, _, _, _, 0],
    ], np.int64),
    np.array([
        [10, 13, 21, 20, 13, 19, 12, 15, 6, 26, 10, 20, 9, _, 11, 18, _, 10, 19, 23, 1, 0, _, _],
        [5, 21, 26, 18, 17, 12, 15, 14, 2, 18, 0, 9, _, 23, 20, 20, 21, _, 4, 7, _, 0, 0, _],
        [19, 20, 4, 22, 11, 7, 13, 11, 14, 20, 16, 17, 22, 15, 0, _, 14, 10, _, 13, 0, _, 0, 0],
        [22, 15, 22, 11, 21, 3, 21, 25, 12, 19, 8, 23, 8, 22, _, 23, 19, 4, 6, _, 1, _, _, 0],
    ], np.int64),
)
del _


class Code:
    """one code of the family: table, K and what of a code word travels"""

    def __init__(self, rate):
        self.rate, self.table, self.k = rate, TABLES[rate], INFO_BYTES[rate]
        self.rows = self.table.shape[0]
        self.m = Z * self.rows                               # checks = parity bits
        self.info_bits = 8 * self.k
        self.first_parity = N - self.m
        self.parity_sent = SENT_BITS - self.info_bits
        # the variables that travel, in the order they are sent; the shortened ones (0, not sent); the punctured parity bits
        self.sent = np.concatenate([np.arange(self.info_bits), self.first_parity + np.arange(self.parity_sent)])
        self.shortened = np.arange(self.info_bits, self.first_parity)
        self.punctured = np.arange(self.first_parity + self.parity_sent, N)
        # per block row: the variables of its 27 checks, [27, degree], edges in table order
        self.layers = []
        for l in range(self.rows):
            cols = np.nonzero(self.table[l] >= 0)[0]
            self.layers.append(np.stack([Z * c + (np.arange(Z) + self.table[l, c]) % Z for c in cols], axis=1))

    def parity_check_matrix(self):
        """H, uint8 [M, 648]"""
        h = np.zeros((self.m, N), np.uint8)
        for l, var in enumerate(self.layers):
            for z in range(Z):
                h[Z * l + z, var[z]] = 1
        return h

    @functools.cached_property
    def _enc(self):
        """P [M, 648 - M] with parity = P x[0 .. 647 - M]"""
        h = self.parity_check_matrix()
        return (lr.gf2_inverse(h[:, self.first_parity:]).astype(np.int64) @ h[:, :self.first_parity].astype(np.int64)) & 1

    def codeword_bits(self, info):
        """info uint8 [n, K] -> x uint8 [n, 648]"""
        info = np.asarray(info, np.uint8).reshape(-1, self.k)
        x = np.zeros((info.shape[0], N), np.uint8)
        x[:, :self.info_bits] = np.unpackbits(info, axis=1, bitorder="little")
        x[:, self.first_parity:] = (x[:, :self.first_parity].astype(np.int64) @ self._enc.T) & 1
        return x

    def encode(self, info):
        """info uint8 [n, K] -> code uint8 [n, 80]: the sent bits, packed LSB first"""
        return np.packbits(self.codeword_bits(info)[:, self.sent], axis=1, bitorder="little")

    def decode(self, llr, max_iter=MAX_ITER):
        """llr int8 [n, 640] (positive = bit 1) -> (bytes uint8 [n, K], iters int32 [n]: the iteration of convergence, 0 = none)"""
        llr = np.asarray(llr, np.int64).reshape(-1, SENT_BITS)
        n = llr.shape[0]
        q = np.zeros((n, N), np.int64)
        q[:, self.sent] = -llr
        q[:, self.shortened] = Q_MAX
        r = [np.zeros((n,) + var.shape, np.int64) for var in self.layers]
        iters = np.zeros(n, np.int32)
        live = np.arange(n)                      # the code words still iterating
        for it in range(1, max_iter + 1):
            if live.size == 0:
                break
            ql = q[live]
            for l, var in enumerate(self.layers):
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
            for var in self.layers:
                ok &= ~(x[:, var].sum(axis=2) & 1).any(axis=1)
            iters[live[ok]] = it
            live = live[~ok]
        out = np.packbits((q[:, :self.info_bits] < 0).astype(np.uint8), axis=1, bitorder="little")
        return out, iters

    # -------------------------------------------------------------------------------------------- the frame stream
    def codewords(self, p):
        return (p + 8 + self.k - 1) // self.k

    def coded_len(self, p):
        return CODE_BYTES * self.codewords(p)

    def info_stream(self, payload):
        p = len(payload)
        s = (p & 0xFFFFFFFF).to_bytes(4, "little") + ((p & 0xFFFFFFFF) ^ 0xFFFFFFFF).to_bytes(4, "little") + bytes(payload)
        s += bytes(self.k * self.codewords(p) - len(s))
        return np.frombuffer(s, np.uint8)

    def stream(self, payload):
        """the byte stream a frame carries behind its 16-byte header"""
        return self.encode(self.info_stream(payload).reshape(-1, self.k)).reshape(-1)

    def row_bytes(self, body_max):
        """the out_stride the decode entry points ask for a body of at most body_max bytes"""
        return max(self.k * (body_max // CODE_BYTES) - 8, 0)

    def receive(self, llr, body, max_iter=MAX_ITER):
        """llr: the LLRs of the stream (LLR 0 = first bit behind the 16-byte header), `body` bytes of it demodulated.
        -> (status, bytes): (HEADER_STATUS, b"") / (UNCORRECTABLE_STATUS, b"") / (0, the delivered bytes)"""
        llr = np.asarray(llr, np.int64)
        nb = body // CODE_BYTES if body > 0 else 0
        if nb == 0:
            return HEADER_STATUS, b""
        head, it = self.decode(llr[:SENT_BITS], max_iter)
        hb = bytes(head[0])
        p, inv = int.from_bytes(hb[:4], "little"), int.from_bytes(hb[4:8], "little")
        if it[0] == 0 or inv != p ^ 0xFFFFFFFF:
            return HEADER_STATUS, b""
        n_cw = min(self.codewords(p), nb)
        out = hb
        if n_cw > 1:
            rest, its = self.decode(llr[SENT_BITS:n_cw * SENT_BITS].reshape(n_cw - 1, SENT_BITS), max_iter)
            if (its == 0).any():
                return UNCORRECTABLE_STATUS, b""
            out += rest.tobytes()
        return 0, out[8:8 + min(p, self.k * nb - 8)]


CODES = tuple(Code(r) for r in RATES)


def code_of_ecc(ecc):
    """the code of a frame mode, with or without the frame check (64 + mode)"""
    return CODES[ECC.index(ecc - 64 if ecc >= 64 else ecc)]
