"""The batched packet decode of ofdm_rx_decode_packets (include/ofdm_hip.h, "every packet of one long capture in one batched decode") as
plain integer rules plus the oracle, shared by tests/test_packets_cpu.py and tests/test_gpu_packets.py.

Input: a capture of n samples and, per packet k, the triple (d_hat_k, f_delta_k, M_k) exactly as ofdm_sc_scan_long returns it.
Notation: L = S, b = sync_backoff.  Packet k is steps 2 - 5 of ofdm_rx_decode_batch on the sub-capture capture[r_k:] with known timing:

    row start      r_k = max(d_hat_k - L - b, 0) & ~1; row-relative peak d_hat_k - r_k; the row's own length n - r_k
    timing fields  rx_prepare_one's rule on that length: off = max(d_hat - L - b, 0) (row-relative), FRAME_SHORT below 10 L samples behind
                   it, ns = min(ceil(len / L) - 10, max_symbols), status -4 if ns * bytes_per_symbol < 16
    CFO            f_delta_k through the context's cfo_mode (off -> 0, abs -> |.|; the wide mode adds 2 pi m / S on the device)
    outputs        bytes, out_len, status: the chain's (orc.decode_given here); offset = r_k + the row's offset; f_delta = what the chain
                   derotated with; metric = M_k bit for bit

On the device the rows are R = min((10 + max_symbols) S + 2, n rounded up to even) samples long, zeros at and beyond sample n, and row k's
own length is len_k = min(R, n - r_k).  `prepare` on len_k and on n - r_k agree (row_rule_is_length_rule: R leaves at least
(10 + max_symbols) L + 1 samples behind a row-relative offset of 0 or 1), which is why the device may cut the rows at R.

Nothing here refers to the slice search of ofdm_rx_decode_long.
"""
import functools
from collections import namedtuple

import numpy as np

import scan_ref
from util import wide

FRAME_OK, FRAME_SHORT, FRAME_NODATA = 0, -1, -4
CFO_OFF, CFO_SIGNED, CFO_ABS = 0, 1, 2

Geometry = namedtuple("Geometry", "r d_rel length row_len")
Prepared = namedtuple("Prepared", "status off ns")


def row_samples(n, S, max_symbols):
    """R: samples of a gathered row (even)"""
    return min((10 + max_symbols) * S + 2, (n + 1) & ~1)


def geometry(n, S, backoff, d_hat, max_symbols):
    """-> Geometry(r_k, d_hat_k - r_k, n - r_k, len_k = min(R, n - r_k))"""
    r = max(d_hat - S - backoff, 0) & ~1
    return Geometry(r, d_hat - r, n - r, min(row_samples(n, S, max_symbols), n - r))


def prepare(length, d_rel, S, backoff, max_symbols, bytes_per_symbol):
    """rx_prepare_one on a capture of `length` samples whose peak is at d_rel -> Prepared(status, trimmed start, live symbols)"""
    off = max(d_rel - S - backoff, 0)
    left = length - off
    if left < 10 * S:
        return Prepared(FRAME_SHORT, off, 0)
    ns = min((left + S - 1) // S - 10, max_symbols)
    if ns * bytes_per_symbol < 16:
        return Prepared(FRAME_NODATA, off, 0)
    return Prepared(FRAME_OK, off, ns)


def cfo_through(f_delta, cfo_mode):
    return 0.0 if cfo_mode == CFO_OFF else abs(f_delta) if cfo_mode == CFO_ABS else f_delta


def row_rule_is_length_rule(n, S, backoff, d_hat, max_symbols, bytes_per_symbol):
    g = geometry(n, S, backoff, d_hat, max_symbols)
    return prepare(g.row_len, g.d_rel, S, backoff, max_symbols, bytes_per_symbol) == prepare(g.length, g.d_rel, S, backoff, max_symbols, bytes_per_symbol)


def packet(orc, x32, d_hat, f_delta, metric, n_fft, guard, mod, max_symbols, backoff=4, cfo_mode=CFO_SIGNED, training=None):
    """The definition for one packet -> dict(status, offset, len, bytes, f_delta, metric, ns, soft): soft = the oracle's equalised points of
    the row (for util.assert_bytes_match; body bit b is stream bit 128 + b).  training: the context's table (None: the default)"""
    S = n_fft + n_fft // 4
    nd = 48 * (n_fft // 64) if guard else n_fft
    g = geometry(len(x32), S, backoff, int(d_hat), max_symbols)
    p = prepare(g.length, g.d_rel, S, backoff, max_symbols, nd * mod // 8)
    fd = cfo_through(float(f_delta), cfo_mode)
    res = {"status": p.status, "offset": g.r + p.off, "len": 0, "bytes": b"", "f_delta": fd, "metric": np.float32(metric), "ns": p.ns, "soft": None}
    if p.status == FRAME_OK:
        w = orc.decode_given(wide(x32[g.r:]), p.off, fd, guard, mod, n_fft, training=training, max_symbols=max_symbols, want_soft=True)
        assert w["status"] == FRAME_OK and w["n_symbols"] == p.ns and w["offset"] == p.off, (w["status"], w["n_symbols"], p)
        res.update(len=len(w["bytes"]), bytes=w["bytes"], soft=w["soft"])
    return res


def packets(orc, x32, det, n_fft, guard, mod, max_symbols, backoff=4, cfo_mode=CFO_SIGNED, training=None):
    """packet() for every row of a scan (anything with d_hat / f_delta / metric sequences)"""
    return [packet(orc, x32, d, fd, m, n_fft, guard, mod, max_symbols, backoff, cfo_mode, training)
            for d, fd, m in zip(det["d_hat"], det["f_delta"], det["metric"])]


# ---------------------------------------------------------------- the captures of the tests
# scan_ref.CAPTURES (16-QAM, guard bands, 15 dB) -> max_symbols: the data symbols of the longer frame, ceil((16 + 560) / 24) and
# ceil((16 + 1400) / 96).  In all three the frame at sample 0 peaks at L + 9 (the channel's delay), so its trimmed start is 5 and the
# rule's clamp max(d_hat - L - b, 0) never acts; "n64_a_cut6" is n64_a less its first 6 samples, where the peak lies at 83 < L + b.
CASES = {"n64_a": 24, "n64_a_cut6": 24, "n64_b": 24, "n256": 15}


@functools.lru_cache(maxsize=None)
def built(orc, name):
    """scan_ref.build_capture, or for name + "_cut6" the same less the capture's first 6 samples """
    if not name.endswith("_cut6"):
        return scan_ref.build_capture(orc, name)
    b = scan_ref.build_capture(orc, name[:-5])
    x = np.ascontiguousarray(b.x[6:])
    return b._replace(name=name, x=x, sums=scan_ref.lag_sums(x, b.L, b.W))


def first_is_clamped(b, d_hat, backoff=4):
    return d_hat[0] - b.S - backoff < 0


def last_is_cut(b, last):
    """the last frame is cut by the capture's end: FRAME_SHORT, or fewer live symbols than the frame was sent with"""
    return last["status"] == FRAME_SHORT or last["ns"] < b.frame_samples[-1] // b.S - 10
