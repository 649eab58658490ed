"""GPU checks of the LDPC(648) modes of rates 2/3, 3/4 and 5/6 (OFDM_ECC_LDPC648_R23 / _R34 / _R56 and their frame-check forms:
k_ldpc_encode<r23|r34|r56>, k_ldpc_decode<r23|r34|r56> and the decode chain around them) against the host functions of the library
and the numpy restatement tests/ldpc_rates_ref.py, which is their definition (parity unpinned by the reference).  Everything compared
is compared bit for bit, iteration counts included: once the LLRs exist nothing here is floating point."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ldpc_rates_ref as rr  # noqa: E402
import ldpc_rates_vectors as rv  # noqa: E402
from chain_checks import (assert_chunking_changes_nothing, assert_entry_points_agree, assert_refuses_short_rows, assert_rows_are,  # noqa: E402
                          ofdm_api as _api)
from tools.link import data_snr as _data_snr, delivered, link as _link, link_on as _link_on  # noqa: E402

pytestmark = pytest.mark.gpu

DECODE_NAMES = ("k_ldpc_decode", "k_ldpc_decode<r23>", "k_ldpc_decode<r34>", "k_ldpc_decode<r56>")
ENCODE_NAMES = ("k_ldpc_encode", "k_ldpc_encode<r23>", "k_ldpc_encode<r34>", "k_ldpc_encode<r56>")
MODES = (41, 42, 43, 105, 106, 107)                    # OFDM_ECC_LDPC648_R23 / _R34 / _R56, and 64 + each


def _rate_of(ecc):
    return rr.ECC.index(ecc - 64 if ecc >= 64 else ecc)


def _ctx(**kw):
    api = _api()
    kw.setdefault("n_fft", 64)
    kw.setdefault("modulation", api.QAM64)
    kw.setdefault("guard_bands", True)
    kw.setdefault("ecc", api.ECC_LDPC648_R34)
    return api.Context(**kw)


def _odd_rows(c, host, dtype):
    """host [n, w] -> a device view [n, w] with an odd row stride on an odd base address"""
    n, w = host.shape
    stride = w + 3 if (w + 3) & 1 else w + 4
    buf = torch.full((n * stride + 1,), 99, dtype=dtype, device=c.device)
    view = buf[1:].view(n, stride)[:, :w]
    view.copy_(torch.from_numpy(host).to(c.device))
    assert view.data_ptr() & 1 and (n == 1 or view.stride(0) & 1)
    return view


def _host_decode(c, rate, llr, max_iter):
    llr = np.ascontiguousarray(llr, np.int8).reshape(-1, rr.SENT_BITS)
    out = np.full((llr.shape[0], rr.INFO_BYTES[rate]), 0xA5, np.uint8)
    iters = np.full(llr.shape[0], -7, np.int32)
    assert c.lib.ofdm_ldpc648_decode_rate(llr.ctypes.data, llr.shape[0], max_iter, rate, out.ctypes.data, iters.ctypes.data) == 0
    return out, iters


# ---------------------------------------------------------------------------------------------------------- 1. the stages
@pytest.mark.parametrize("max_iter", rv.MAX_ITERS)
@pytest.mark.parametrize("n_cw", [1, 2, 3])
@pytest.mark.parametrize("rate", rr.RATES)
def test_decoder_stage_is_the_host_decoder(rate, n_cw, max_iter):
    """9 rows (more than one workgroup's four wavefronts) of 1, 2 and 3 code words (the lone and the odd last one) of the shared pool:
    clean words, words inside the waterfall, hopeless words and the saturated corners, a word that converges at once side by side
    with one that never does on either half.  All K bytes are compared, bytes 64 .. 66 of rate 5/6 included."""
    c = _ctx()
    k = rr.INFO_BYTES[rate]
    llr, want, want_it = rv.rows(rate, 9, n_cw, max_iter)
    host, host_it = _host_decode(c, rate, llr, max_iter)
    np.testing.assert_array_equal(host_it, want_it)
    np.testing.assert_array_equal(host, want)
    if n_cw >= 2:                                           # side by side: (at once, never) and (never, at once)
        pairs = {(int(a), int(b)) for a, b in want_it.reshape(9, n_cw)[:, :2]}
        assert (1, 0) in pairs and (0, 1) in pairs
    dev = _odd_rows(c, llr, torch.int8)
    first = None
    for cap in (0, 1, 3):                                  # the device-sized grid, then one and three workgroups for every frame
        c.set_tuning("grid_cap", cap)
        got, its = c.ldpc_decode(dev, max_iter=max_iter, rate=rate)
        c.synchronize()
        assert c.last_dispatch() == DECODE_NAMES[rate]
        assert got.shape == (9, k * n_cw) and its.shape == (9, n_cw)
        np.testing.assert_array_equal(its.cpu().numpy().reshape(-1), host_it, err_msg=str(cap))
        np.testing.assert_array_equal(got.cpu().numpy().reshape(-1, k), host, err_msg=str(cap))
        first = got if first is None else first
        assert torch.equal(first, got)
    c.set_tuning("grid_cap", 0)


@pytest.mark.parametrize("rate", rr.RATES)
def test_encoder_stage_is_the_host_encoder(rate):
    c = _ctx()
    k = rr.INFO_BYTES[rate]
    for n_frames, n_cw in ((9, 1), (9, 2), (9, 3), (70, 5)):   # 350 code words: more than one workgroup of one thread each
        info = np.random.default_rng(n_frames * 100 + n_cw + rate).integers(0, 256, (n_frames, k * n_cw), dtype=np.uint8)
        info[0, :k] = np.arange(k)
        host = np.zeros((n_frames * n_cw, 80), np.uint8)
        flat = np.ascontiguousarray(info.reshape(-1, k))
        assert c.lib.ofdm_ldpc648_encode_rate(flat.ctypes.data, flat.shape[0], rate, host.ctypes.data) == 0
        np.testing.assert_array_equal(host, rr.CODES[rate].encode(flat))
        for cap in (0, 1):
            c.set_tuning("grid_cap", cap)
            got = c.ldpc_encode(_odd_rows(c, info, torch.uint8), rate=rate)
            c.synchronize()
            assert c.last_dispatch() == ENCODE_NAMES[rate] and got.shape == (n_frames, 80 * n_cw)
            np.testing.assert_array_equal(got.cpu().numpy().reshape(-1, 80), host)
        c.set_tuning("grid_cap", 0)


def test_rate_0_through_the_rate_calls_is_the_existing_stage():
    c = _ctx()
    llr, _, _ = rv.rows(0, 9, 3, 20)
    dev = torch.from_numpy(llr).to(c.device)
    a, ai = c.ldpc_decode(dev)
    out = torch.zeros((9, 120), dtype=torch.uint8, device=c.device)
    it = torch.zeros((9, 3), dtype=torch.int32, device=c.device)
    assert c.lib.ofdm_ldpc648_decode_rate_batch(c.h, dev.data_ptr(), 9, 1920, 3, 20, 0, out.data_ptr(), 120, it.data_ptr()) == 0
    c.synchronize()
    assert c.last_dispatch() == "k_ldpc_decode" and torch.equal(a, out) and torch.equal(ai, it)
    info = a.contiguous()
    code = torch.zeros((9, 240), dtype=torch.uint8, device=c.device)
    assert c.lib.ofdm_ldpc648_encode_rate_batch(c.h, info.data_ptr(), 9, 120, 3, 0, code.data_ptr(), 240) == 0
    c.synchronize()
    assert c.last_dispatch() == "k_ldpc_encode" and torch.equal(code, c.ldpc_encode(info))


@pytest.mark.parametrize("rate", (1, 2, 3))
def test_stage_argument_checks(rate):
    c = _ctx()
    k = rr.INFO_BYTES[rate]
    llr = torch.zeros((2, 1280), dtype=torch.int8, device=c.device)
    out = torch.full((2, 2 * k), 7, dtype=torch.uint8, device=c.device)
    it = torch.full((4,), -9, dtype=torch.int32, device=c.device)
    d = c.lib.ofdm_ldpc648_decode_rate_batch
    assert d(c.h, llr.data_ptr(), 2, 1280, 2, 20, rate, out.data_ptr(), 2 * k, it.data_ptr()) == 0
    assert d(c.h, llr.data_ptr(), 2, 1280, 2, 20, rate, out.data_ptr(), 2 * k, None) == 0         # iters is optional
    assert d(c.h, llr.data_ptr(), 2, 1279, 2, 20, rate, out.data_ptr(), 2 * k, None) == -1        # llr_stride below 640 n_cw
    assert d(c.h, llr.data_ptr(), 2, 1280, 2, 20, rate, out.data_ptr(), 2 * k - 1, None) == -1    # out_stride below K n_cw
    for bad in (0, -1, 65):
        assert d(c.h, llr.data_ptr(), 2, 1280, 2, bad, rate, out.data_ptr(), 2 * k, None) == -1
    for bad in (-1, 4):
        assert d(c.h, llr.data_ptr(), 2, 1280, 2, 20, bad, out.data_ptr(), 2 * k, None) == -1
    assert d(c.h, llr.data_ptr(), -1, 1280, 2, 20, rate, out.data_ptr(), 2 * k, None) == -1
    assert d(c.h, None, 2, 1280, 2, 20, rate, out.data_ptr(), 2 * k, None) == -1
    assert d(None, llr.data_ptr(), 2, 1280, 2, 20, rate, out.data_ptr(), 2 * k, None) == -1
    c.synchronize()
    assert it.tolist() == [1, 1, 1, 1] and not out.any()    # all-zero LLRs converge at once to zeros
    out.fill_(7); it.fill_(-9)
    assert d(c.h, None, 0, 1280, 2, 20, rate, None, 2 * k, None) == 0
    assert d(c.h, llr.data_ptr(), 2, 0, 0, 20, rate, out.data_ptr(), 0, it.data_ptr()) == 0
    e = c.lib.ofdm_ldpc648_encode_rate_batch
    info = torch.zeros((2, 2 * k), dtype=torch.uint8, device=c.device)
    code = torch.full((2, 160), 7, dtype=torch.uint8, device=c.device)
    assert e(c.h, info.data_ptr(), 2, 2 * k - 1, 2, rate, code.data_ptr(), 160) == -1
    assert e(c.h, info.data_ptr(), 2, 2 * k, 2, rate, code.data_ptr(), 159) == -1
    assert e(c.h, info.data_ptr(), 2, 2 * k, 2, 4, code.data_ptr(), 160) == -1
    assert e(c.h, None, 2, 2 * k, 2, rate, code.data_ptr(), 160) == -1
    assert e(c.h, None, 0, 2 * k, 2, rate, None, 160) == 0 and e(c.h, info.data_ptr(), 2, 0, 0, rate, code.data_ptr(), 0) == 0
    c.synchronize()
    assert (out == 7).all() and (it == -9).all() and (code == 7).all()   # zero counts write nothing
    assert e(c.h, info.data_ptr(), 2, 2 * k, 2, rate, code.data_ptr(), 160) == 0
    c.synchronize()
    assert not code.any()


# ---------------------------------------------------------------------------------------------------------- helpers of the chain tests
def _reference_decode(c, code, rx, r, max_symbols, frame_len=None):
    """per frame that reached the demodulator: (status, out_len, bytes) by the rule of the header -- ldpc_rates_ref's receive over the
    LLRs rx_llr returns for the frame at OFDM_SOFT_LLR_SCALE with the context's channel estimate, from LLR 128 on"""
    frame_len = rx.shape[1] if frame_len is None else frame_len
    hk = c.estimate_channel(rx, r["offset"], r["f_delta"], frame_len=frame_len)
    L = c.rx_llr(rx, max_symbols, first_symbol=10, offset=r["offset"], f_delta=r["f_delta"], hk=hk, frame_len=frame_len)
    c.synchronize()
    L = L.cpu().numpy()
    want = {}
    for f in range(rx.shape[0]):
        if int(r["status"][f]) not in (0, rr.HEADER_STATUS, rr.UNCORRECTABLE_STATUS):
            continue
        nsym = min(-(-(frame_len - int(r["offset"][f])) // c.S) - 10, max_symbols)      # k_rx_prepare's live symbols
        body = nsym * c.bytes_per_symbol - 16
        st, data = code.receive(L[f, 128:], body)
        want[f] = (st, len(data), data)
    return want


# ---------------------------------------------------------------------------------------------------------- 2. payloads through the chain
@pytest.mark.parametrize("ecc", MODES)
def test_ragged_payloads_come_back_whole(ecc):
    """N = 64, 64-QAM, guard bands, 30 dB: payloads at every edge of the frame stream (0, 1, K - 8 and K - 7 around one code word, 2 K - 8,
    560), each with its own frame length"""
    api = _api()
    rate, fcs = _rate_of(ecc), ecc >= 64
    code = rr.CODES[rate]
    k = code.k
    c = _ctx(ecc=ecc)
    for p in (0, 1, k - 8, k - 7, 2 * k - 8, 560):
        assert c.coded_len(p) == code.coded_len(p + (8 if fcs else 0))
        pay, rx = _link_on(c, 3, p, 30.0, 400 + p)
        D = c.data_symbols(p)
        r = c.decode_batch(rx, max_symbols=D)
        c.synchronize()
        dc = c.last_dispatch()
        assert "k_sym<llr>" in dc and DECODE_NAMES[rate] in dc.split("+") and "k_viterbi" not in dc and dc.endswith("k_fcs_check") == fcs, dc
        assert r["status"].tolist() == [0, 0, 0] and r["len"].tolist() == [p] * 3, (p, r["status"].tolist(), r["len"].tolist())
        assert torch.equal(r["bytes"][:, :p], pay), p
        c.encode_batch(pay)
        assert ENCODE_NAMES[rate] in c.last_dispatch().split("+") and c.last_dispatch().startswith("k_fcs_wrap") == fcs, c.last_dispatch()
    assert (c.coded_len(560) // 80, c.frame_samples(560)) == {41: (11, 2800), 42: (10, 2640), 43: (9, 2480),
                                                               105: (11, 2800), 106: (10, 2640), 107: (9, 2480)}[ecc]


@pytest.mark.parametrize("ecc", MODES)
def test_every_decode_entry_point(ecc):
    api = _api()
    rate, fcs = _rate_of(ecc), ecc >= 64
    code = rr.CODES[rate]
    c, pay, rx, D = _link(ecc, 64, 6, 4, 560, 30.0, 77)
    r, ones = assert_entry_points_agree(api, c, rx, D, dict(ecc=rr.ECC[rate], fcs=fcs))
    assert (r["status"] == 0).all() and (r["len"] == 560).all() and torch.equal(r["bytes"][:, :560], pay)
    for f, one in enumerate(ones):                           # every entry point agreed with the one-row decode: that is the payload
        assert one == (0, 560, int(r["offset"][f]), bytes(pay[f].cpu().numpy())), f
    assert api.decode_long(rx[0].cpu().numpy(), True, api.QAM64, ecc=rr.ECC[rate], fcs=fcs)["len"] == 560
    msg = b"four rates on one graph family"
    assert api.decode(api.encode(msg, True, api.QAM16, ecc=rr.ECC[rate], fcs=fcs), True, api.QAM16, ecc=rr.ECC[rate], fcs=fcs) == msg
    # a row too short for what the chain can write is refused; decode_batch's own rows are long enough
    need = code.row_bytes(D * c.bytes_per_symbol - 16) - (8 if fcs else 0)
    assert c.decode_row_bytes(D) == need
    assert assert_refuses_short_rows(c, rx, D, need, accepts=True) == [560, 0]


@pytest.mark.parametrize("ecc,chest", [(42, 0), (107, 1)])
def test_chain_at_n_1024(ecc, chest):
    rate = _rate_of(ecc)
    c, pay, rx, D = _link(ecc, 1024, 6, 3, 1304, _data_snr(1024, 30.0), 31, chest_mode=chest)
    r = c.decode_batch(rx, max_symbols=D)
    c.synchronize()
    dc = c.last_dispatch()
    assert DECODE_NAMES[rate] in dc.split("+") and ("k_chest_solve" in dc) == bool(chest), dc
    assert r["status"].tolist() == [0, 0, 0] and r["len"].tolist() == [1304] * 3 and torch.equal(r["bytes"][:, :1304], pay)


# ---------------------------------------------------------------------------------------------------------- 3. bad frames
def _forged_rows(code):
    k = code.k
    rng = np.random.default_rng(70 + code.rate)
    pay = rng.integers(0, 256, 2 * k + 20, dtype=np.uint8).tobytes()     # 3 code words
    info = code.info_stream(pay).reshape(-1, k)
    assert info.shape[0] == 3
    good = code.encode(info).reshape(-1)

    def with_len(p, inv=None):
        i = info.copy()
        i[0, :4] = np.frombuffer((p & 0xFFFFFFFF).to_bytes(4, "little"), np.uint8)
        i[0, 4:8] = np.frombuffer(((p ^ 0xFFFFFFFF) if inv is None else inv).to_bytes(4, "little"), np.uint8)
        return code.encode(i).reshape(-1)

    junk = rng.integers(0, 256, 80, dtype=np.uint8)
    rows = {"valid": good,
            "cw0 random": np.concatenate([junk, good[80:]]),
            "not complementary": with_len(len(pay), len(pay) ^ 0xFFFFFFEF),
            "later cw random": np.concatenate([good[:160], junk]),
            "p beyond the frame": with_len(1000),
            "p = 2^32 - 1": with_len(0xFFFFFFFF),
            "short p": np.concatenate([with_len(20)[:80], junk, junk])}
    return pay, rows


@pytest.mark.parametrize("rate", (1, 2, 3))
def test_every_status_branch_deterministically(rate):
    """forged streams sent through an OFDM_ECC_NONE context: a capture cut inside the body delivers the prefix min(p, K nb - 8), forged
    length words give OFDM_FRAME_HEADER, a later code word replaced by noise gives OFDM_FRAME_UNCORRECTABLE with out_len 0; and every
    row is what ldpc_rates_ref makes of the device's own LLRs"""
    api = _api()
    code = rr.CODES[rate]
    k = code.k
    u = _ctx(ecc=api.ECC_NONE)
    c = _ctx(ecc=rr.ECC[rate])
    pay, rows = _forged_rows(code)
    p = len(pay)
    names = list(rows)
    tx = u.encode_batch(torch.from_numpy(np.stack([rows[n] for n in names])).to(u.device))
    rx = u.channel_batch(tx, snr_db=40.0, seed=7, span=tx.shape[1] + 160)
    D = c.data_symbols(p)
    assert D == u.data_symbols(240) and D * c.bytes_per_symbol - 16 >= 240
    seen = set()
    S = c.S
    cases = [("whole", D, rx.shape[1]), ("capture cut mid-frame", D, 8 + 15 * S + S // 2), ("max_symbols cut", 5, rx.shape[1]),
             ("body < 80", 2, rx.shape[1])]
    for what, syms, frame_len in cases:
        cap = rx[:, :frame_len].contiguous()
        for _ in range(2):                                   # deterministically
            r = c.decode_batch(cap, max_symbols=syms)
            c.synchronize()
            want = _reference_decode(c, code, cap, r, syms)
            assert len(want) == len(names), what
            assert_rows_are(r, want)
        st = dict(zip(names, r["status"].tolist()))
        ln = dict(zip(names, r["len"].tolist()))
        seen |= set(st.values())
        if what == "whole":
            assert st == {"valid": 0, "cw0 random": api.FRAME_HEADER, "not complementary": api.FRAME_HEADER,
                          "later cw random": api.FRAME_UNCORRECTABLE, "p beyond the frame": 0, "p = 2^32 - 1": 0, "short p": 0}, st
            assert (ln["valid"], ln["p beyond the frame"], ln["p = 2^32 - 1"], ln["short p"]) == (p, 3 * k - 8, 3 * k - 8, 20)
            assert ln["later cw random"] == 0 and ln["cw0 random"] == 0
            assert bytes(r["bytes"][0, :p].cpu().numpy()) == pay and bytes(r["bytes"][6, :20].cpu().numpy()) == pay[:20]
        elif what == "body < 80":
            assert set(st.values()) == {api.FRAME_HEADER} and not any(ln.values())
        else:                                                # two whole code words are left: the prefix, and the junk behind the cut unseen
            cut = 2 * k - 8
            assert st["valid"] == 0 and ln["valid"] == cut and bytes(r["bytes"][0, :cut].cpu().numpy()) == pay[:cut], (what, st, ln)
            assert st["later cw random"] == 0 and ln["later cw random"] == cut
    assert seen == {0, api.FRAME_HEADER, api.FRAME_UNCORRECTABLE}, seen


# ---------------------------------------------------------------------------------------------------------- 4. chain = reference
# dB at which this 12-frame link (seeds 6, 7, 8) leaves frames of the mode in all three states: seen on an MI355X with chest_mode 0 at
# 7 / 9 / 10 dB: rate 2/3 eight frames delivered and four reported (-4 and -5 both), rate 3/4 nine and three, rate 5/6 six and six;
# one dB lower at most a third are delivered, two dB higher all or all but two.  With chest_mode 1 the same points deliver 12, 12 and
# 11 of 12: the equality with the reference is what is asserted there, not the mix
NOISY_SNR_DB = {1: 7.0, 2: 9.0, 3: 10.0}


@pytest.mark.parametrize("chest", [0, 1])
@pytest.mark.parametrize("rate", (1, 2, 3))
def test_chain_is_the_reference_over_the_devices_own_llrs(rate, chest):
    """exact: the delivered bytes and statuses are what ldpc_rates_ref makes of the LLRs the device itself computed"""
    code = rr.CODES[rate]
    for snr in (30.0, NOISY_SNR_DB[rate]):
        c, pay, rx, D = _link(rr.ECC[rate], 64, 6, 12, 400, snr, 5 + rate, chest_mode=chest)
        r = c.decode_batch(rx, max_symbols=D)
        c.synchronize()
        assert DECODE_NAMES[rate] in c.last_dispatch().split("+") and ("k_chest_solve" in c.last_dispatch()) == bool(chest)
        want = _reference_decode(c, code, rx, r, D)
        good = [f for f, (st, n_out, data) in want.items() if st == 0 and data == bytes(pay[f].cpu().numpy())]
        print(f"rate {rate}, chest {chest}, {snr} dB: statuses {r['status'].tolist()}, {len(good)} of 12 whole")
        assert len(want) == 12 and (len(good) == 12 or snr < 30.0)
        if snr < 30.0 and not chest:                         # the point is a noisy one: delivered and reported frames side by side
            assert 0 < len(good) < 12 and set(r["status"].tolist()) == {0, -4, -5}
        assert_rows_are(r, want)
        assert_rows_are(assert_chunking_changes_nothing(c, rx, D, r), want)   # many chunks of the LLR workspace


# ---------------------------------------------------------------------------------------------------------- 5. one link, both rate-3/4 modes
# N = 64, 64-QAM, guard bands, payload 560, 256 frames, seed 9012, the same payloads, delays, CFO and channel seed for
# OFDM_ECC_CONV_K7F_R34 and OFDM_ECC_LDPC648_R34.  The point was not chosen for its outcome: 12 dB is the highest point of the sweep of
# tools/bench_ldpc_rates.py (profiles/ldpc_rates_ber_and_speed.json, 4 096 frames a point) at which K7F_R34 delivers fewer than 90 %
# whole (3 588 right / 508 wrong with status 0 / 0 reported there, 3 939 / 157 / 0 at 13 dB; LDPC648_R34 4 096 / 0 / 0 at both).
# Seen on an MI355X over THIS link (right / wrong / reported of 256; the record's "point" block):
#     11 dB   K7F_R34 169 / 87 / 0    LDPC648_R34 253 / 0 / 3
#     12 dB   K7F_R34 214 / 42 / 0    LDPC648_R34 256 / 0 / 0
#     13 dB   K7F_R34 238 / 18 / 0    LDPC648_R34 256 / 0 / 0
# Asserted at 12 dB: each mode's count of whole frames lies between its counts at the neighbouring points (169 .. 238 and 253 .. 256),
# LDPC648_R34 reports at most the 3 frames it reports at 11 dB, delivers at least as many frames whole as K7F_R34, and -- what the mode
# must show wherever it stands -- delivers no frame with status 0 and a wrong length or wrong bytes.
POINT_SNR_DB, POINT_SEED = 12.0, 9012


def test_ldpc_r34_against_the_framed_viterbi_r34_on_one_link():
    api = _api()
    res = {}
    for ecc in (api.ECC_CONV_K7F_R34, api.ECC_LDPC648_R34):
        c, pay, rx, D = _link(ecc, 64, 6, 256, 560, POINT_SNR_DB, POINT_SEED)
        r = c.decode_batch(rx, max_symbols=D)
        c.synchronize()
        right, ok = delivered(r, pay, 560)
        res[ecc] = (pay, int(right.sum()), int((ok & ~right).sum()), int((~ok).sum()))
    assert torch.equal(res[api.ECC_CONV_K7F_R34][0], res[api.ECC_LDPC648_R34][0])        # the same payloads
    _, k_right, k_wrong, k_reported = res[api.ECC_CONV_K7F_R34]
    _, l_right, l_wrong, l_reported = res[api.ECC_LDPC648_R34]
    print(f"{POINT_SNR_DB} dB, 256 frames, right / wrong / reported: K7F_R34 {k_right} / {k_wrong} / {k_reported}, "
          f"LDPC648_R34 {l_right} / {l_wrong} / {l_reported}")
    assert 169 <= k_right <= 238, k_right                    # seen: 214 (42 more with status 0 and damaged bytes)
    assert 253 <= l_right <= 256, l_right                    # seen: 256
    assert l_reported <= 3 and l_right + l_reported == 256   # seen: 0 reported
    assert l_wrong == 0                                      # failures are reported, never delivered
    assert l_right >= k_right
