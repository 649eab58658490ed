"""One reference receiver for any row of tests/cover_cases.py, put together from what the suite already defines -- nothing here is
new mathematics.  Shared by tests/test_cover_cpu.py and tests/test_gpu_cover.py.

    mode_encode     payload -> the byte stream a frame of mode ecc carries behind its 16-byte header: fcs_ref.wrap, the host RS encoder
                    (rs_vectors.host_encode), then the inner code (oracle.hamming74_encode, conv_ref.encode, framed_ref.encode_stream,
                    ldpc_rates_ref's stream); its length is chain_refs.mode_coded_len
    front_end       per frame (status, offset, live symbols, d_hat, f_delta, metric) in f64: orc.sc_sync + packets_ref.prepare +
                    packets_ref.cfo_through (+ cfo_wide_ref.cfo_wide), or orc.decode_ref's timing under SYNC_REFERENCE
    hard_reference  bytes and equalised points of a hard inner mode: orc.decode_given under LS, orc.cfo_rotate + orc.estimate_channel +
                    chest_ref.smooth + orc.rx_demod under WLS
    outer_layers    the CPU rule of the outer layers over an inner row: rs_vectors.host_row, then fcs_ref.check
    compose         a soft inner mode from the stage entry points of a context that knows none of the row's options, given the
                    chain's offset / f_delta, then the CPU decoder of the mode and outer_layers.  Every stage is pinned to its own
                    f64 reference (tests/test_gpu_llr_oracle.py, _chest, _cfo_wide, _noise_weight), which is why the composition may
                    be exact where an end-to-end f64 receiver could not: 0.4 - 4 % of int8 LLRs lie within soft_ref.llr_eps of a
                    rounding boundary.
"""
from collections import namedtuple

import numpy as np

import cfo_wide_ref
import chain_refs
import chest_ref
import conv_ref
import cover_cases as cc
import fcs_ref
import framed_ref
import ldpc_rates_ref as lrr
import packets_ref as P
import rs_vectors as rv
import soft_ref as sr
from util import header_rule, wide

FRAME_OK, FRAME_SHORT, FRAME_NOSYNC, FRAME_BADTIMING, FRAME_HEADER, FRAME_UNCORRECTABLE, FRAME_FCS = 0, -1, -2, -3, -4, -5, -6
HARD_INNER = (0, 1)

Front = namedtuple("Front", "status offset nsym d_hat f_delta metric")


def host_lib():
    """the library's host entry points (the RS codec): no device needed"""
    from ofdm_amd import _lib

    return _lib.load()


# ---------------------------------------------------------------------------------------------------------- transmit
def inner_encode(inner, data: bytes) -> bytes:
    if inner == 0:
        return bytes(data)
    if inner in (1, 2):
        from oracle import oracle as orc

        return orc.hamming74_encode(data)
    if inner == 5:
        return bytes(conv_ref.encode(data))
    if inner in lrr.ECC:
        return bytes(lrr.code_of_ecc(inner).stream(data))
    return bytes(framed_ref.encode_stream(data, inner - 10))


def mode_encode(ecc, payload: bytes) -> bytes:
    fcs, rs, inner = chain_refs.mode_layers(ecc)
    data = bytes(payload)
    if fcs:
        data = fcs_ref.wrap(data)
    if rs:
        data = rv.host_encode(host_lib(), data)
    return inner_encode(inner, data)


# ---------------------------------------------------------------------------------------------------------- front end
def _prepare_ref(n, off, S, max_symbols, bytes_per_symbol):
    """k_rx_prepare_ref (src/receiver.rs:21-36) -> (status, live symbols)"""
    if off < 0 or off > n:
        return FRAME_BADTIMING, 0
    left = n - off
    if left < 10 * S:
        return FRAME_SHORT, 0
    ns = min((left + S - 1) // S - 10, max_symbols)
    return (FRAME_HEADER, 0) if ns * bytes_per_symbol < 16 else (FRAME_OK, ns)


def front_end(orc, rx, k, max_symbols, backoff=None):
    """rx [frames, span] complex64, k: cover_cases.Case -> [Front] per frame.  backoff: another one than the row's (mutation checks)"""
    backoff = k.backoff if backoff is None else backoff
    out = []
    trn = orc.default_training(k.n)
    for x32 in rx:
        x = wide(x32)
        if k.sync_mode == cc.REFERENCE:
            w = orc.decode_ref(x, k.guard, k.mod, k.n)
            off = int(w["offset"])
            st, ns = _prepare_ref(x.size, off, k.S, max_symbols, k.bytes_per_symbol)
            if st != FRAME_OK or k.cfo_mode == cc.CFO_OFF:
                fd = 0.0
            else:
                fd = orc.frequency_correction(x[off + 3 * k.S:off + 4 * k.S], x[off + 4 * k.S:off + 5 * k.S])
            out.append(Front(st, off, ns, off + 1, fd, w["metric"]))
            continue
        d, _, metric, fd = orc.sc_sync(x, L=k.S, window_reps=k.reps, n_lags=k.n_lags, threshold=k.threshold)
        if d < 0:
            out.append(Front(FRAME_NOSYNC, 0, 0, d, 0.0, metric))
            continue
        p = P.prepare(x.size, d, k.S, backoff, max_symbols, k.bytes_per_symbol)
        fd = P.cfo_through(fd, P.CFO_SIGNED if k.cfo_mode == cc.CFO_WIDE else k.cfo_mode)
        if k.cfo_mode == cc.CFO_WIDE:
            _, wfd, _ = cfo_wide_ref.cfo_wide(x, k.n, trn, [p.off], [fd], span=8, status=[p.status])
            fd = float(wfd[0])
        out.append(Front(p.status, p.off, p.ns, d, fd, metric))
    return out


# ---------------------------------------------------------------------------------------------------------- hard inner modes
def hard_reference(orc, x32, k, offset, f_delta, max_symbols):
    """-> (body bytes the header rule keeps, equalised points of the whole stream, header included) for a frame of status 0"""
    x = wide(x32)
    if k.chest_mode == cc.LS:
        w = orc.decode_given(x, offset, f_delta, k.guard, k.mod, k.n, max_symbols=max_symbols, want_soft=True)
        assert w["status"] == FRAME_OK, w["status"]
        return w["bytes"], w["soft"]
    trn = orc.default_training(k.n)
    ns = min((x.size - offset + k.S - 1) // k.S - 10, max_symbols)
    buf = np.zeros((10 + ns) * k.S, np.complex128)
    live = min(buf.size, x.size - offset)
    buf[:live] = x[offset:offset + live]
    rot = orc.cfo_rotate(buf, f_delta, 0)
    hk = chest_ref.smooth(orc.estimate_channel(rot[5 * k.S:10 * k.S], trn, k.n), trn, k.n)
    stream, soft = orc.rx_demod(rot[10 * k.S:], k.n, k.guard, k.mod, hk=hk, want_soft=True)
    assert len(stream) >= 16
    keep = header_rule(*chain_refs.header_of(np.frombuffer(stream, np.uint8)), len(stream) - 16)
    return stream[16:16 + keep], soft


def hard_finish(orc, inner, body: bytes) -> bytes:
    """what a hard inner mode delivers of the body the header rule kept"""
    return body if inner == 0 else orc.hamming74_decode(body[:len(body) // 7 * 7])[0]


def outer_layers(ecc, status, data: bytes):
    """(status, bytes) of the outer layers of mode ecc over an inner row"""
    fcs, rs, _ = chain_refs.mode_layers(ecc)
    if status == FRAME_OK and rs:
        out, out_len, fixed = rv.host_row(host_lib(), np.frombuffer(data, np.uint8), len(data))
        status, data = (FRAME_UNCORRECTABLE, b"") if fixed < 0 else (FRAME_OK, bytes(out[:out_len]))
    if status == FRAME_OK and fcs:
        inside = fcs_ref.check(data)
        status, data = (FRAME_FCS, b"") if inside is None else (FRAME_OK, bytes(inside))
    return int(status), (data if status == FRAME_OK else b"")


# ---------------------------------------------------------------------------------------------------------- soft inner modes
def soft_finish(inner, llr_row, hard_row, body):
    """(status, bytes) of a soft inner mode over the LLRs of the frame's data symbols (and, for the modes whose length travels in the
    16-byte header, its hard bytes)"""
    if inner in (2, 5):
        lo, hi = chain_refs.header_of(hard_row)
        keep = header_rule(lo, hi, body)
        if inner == 2:
            return FRAME_OK, bytes(sr.ham_decode_soft(llr_row[128:128 + 56 * (keep // 7)]))
        n_out = max(keep // 2 - 1, 0)
        return FRAME_OK, bytes(conv_ref.viterbi(llr_row[128:128 + 8 * keep], terminated=(hi == 0 and lo <= body))[:n_out])
    if inner in lrr.ECC:
        return lrr.code_of_ecc(inner).receive(llr_row[128:], body, lrr.MAX_ITER)
    return framed_ref.decode_stream(llr_row[128:128 + 8 * body], body, inner - 10)


def stages(s, rx, k, status, offset, f_delta, max_symbols):
    """the stage entry points of `s`, a context of the row's n_fft / modulation / guard_bands and nothing else, at the chain's offset /
    f_delta: estimate_channel, chest_smooth under WLS, noise_bins under LLRW_NOISE, then rx_llr and rx_demod
    -> (LLRs int8 [frames, .], hard bytes uint8 [frames, .], the device's channel estimate)"""
    import torch

    st = torch.as_tensor(np.asarray(status, np.int32), device=s.device)
    off = torch.where(st == 0, offset, torch.zeros_like(offset))
    hk = s.estimate_channel(rx, off, f_delta)
    if k.chest_mode == cc.WLS:
        hk = s.chest_smooth(hk)
    q = s.noise_bins(rx, off, f_delta, st)["weight"] if k.llr_weight == cc.LLRW_NOISE else None
    llr = s.rx_llr(rx, max_symbols, first_symbol=10, offset=off, f_delta=f_delta, hk=hk, bin_weight=q)
    hard = s.rx_demod(rx, max_symbols, first_symbol=10, offset=off, f_delta=f_delta, hk=hk)
    s.synchronize()
    return llr.cpu().numpy(), hard.cpu().numpy(), hk


def compose(s, rx, k, status, offset, f_delta, max_symbols):
    """{frame: (status, out_len, bytes)} a soft row must deliver; status: the front end's, offset / f_delta: the chain's tensors"""
    L, H, _ = stages(s, rx, k, status, offset, f_delta, max_symbols)
    body = max_symbols * k.bytes_per_symbol - 16
    want = {}
    for f, st in enumerate(status):
        if st != FRAME_OK:
            want[f] = (int(st), 0, b"")
            continue
        st, data = soft_finish(k.inner, L[f], H[f], body)
        st, data = outer_layers(k.ecc, st, data if st == FRAME_OK else b"")
        want[f] = (st, len(data), data)
    return want
