"""GPU checks of the punctured rates and the framed convolutional modes (OFDM_ECC_CONV_K7F_R12 / _R23 / _R34: k_conv_encode_p,
k_viterbi_k7f and the decode chain around them) against the numpy restatement tests/framed_ref.py, which is their definition (parity
unpinned by the reference).  Everything compared with it is compared bit for bit: once the LLRs exist nothing here is floating point."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_ref as cr  # noqa: E402
import framed_ref as fr  # noqa: E402
from chain_checks import (assert_chunking_changes_nothing, assert_entry_points_agree, assert_refuses_short_rows, assert_rows_are,  # noqa: E402
                          ofdm_api as _api)
from chain_refs import decoder_rows as _decoder_rows  # noqa: E402
from tools.link import data_snr as _data_snr, delivered, link as _link  # noqa: E402

pytestmark = pytest.mark.gpu

RATES = (0, 1, 2)


def _framed(rate):
    return _api().ECC_CONV_K7F_R12 + rate


def _ctx(**kw):
    api = _api()
    kw.setdefault("n_fft", 64)
    kw.setdefault("modulation", api.QAM64)
    kw.setdefault("guard_bands", True)
    kw.setdefault("ecc", api.ECC_CONV_K7F_R12)
    return api.Context(**kw)


# ---------------------------------------------------------------------------------------------------------- 1. the encoder stage
@pytest.mark.parametrize("n_bytes", [0, 1, 2, 3, 63, 64, 560, 1304])
def test_punctured_encoder_matches_the_restatement(n_bytes):
    c = _ctx()
    rng = np.random.default_rng(300 + n_bytes)
    F = 5
    wide = rng.integers(0, 256, (F, n_bytes + 7), dtype=np.uint8)
    dev = torch.from_numpy(wide).to(c.device)
    for rate in RATES:
        got = c.conv_encode(dev[:, :n_bytes], rate=rate)               # a row stride larger than the row
        c.synchronize()
        assert c.last_dispatch() == "k_conv_encode_p"
        assert got.shape == (F, fr.body_len(n_bytes, rate))
        for f in range(F):
            np.testing.assert_array_equal(got[f].cpu().numpy(), fr.encode_punctured(wide[f, :n_bytes].tobytes(), rate), err_msg=str((rate, f)))
        if rate == 0:
            assert torch.equal(got, c.conv_encode(dev[:, :n_bytes]))
        f_ = c.lib.ofdm_conv_k7_encode_punctured
        assert f_(c.h, dev.data_ptr(), F, n_bytes - 1, n_bytes, rate, got.data_ptr(), got.shape[1]) == -1
        assert f_(c.h, dev.data_ptr(), F, n_bytes + 7, n_bytes, rate, got.data_ptr(), got.shape[1] - 1) == -1
    assert c.lib.ofdm_conv_k7_encode_punctured(c.h, dev.data_ptr(), F, n_bytes + 7, n_bytes, 3, got.data_ptr(), 4 * n_bytes + 8) == -1


# ---------------------------------------------------------------------------------------------------------- 2. the decoder stage
@pytest.mark.parametrize("n_steps", [0, 8, 13, 48, 64, 65, 1000, 4488, 10440])
def test_punctured_decoder_matches_the_restatement(n_steps):
    c = _ctx()
    c.set_tuning("grid_cap", 2)                                   # 8 wavefronts: every one of them decodes several frames
    rng = np.random.default_rng(400 + n_steps)
    full, _ = _decoder_rows(rng, n_steps, 10 if n_steps < 4000 else 6)   # noisy codewords, uniform int8, all zero, saturated codewords
    F = full.shape[0]
    for rate in RATES:
        keep = fr.keep_mask(n_steps, rate)
        rows = full[:, keep]
        assert rows.shape[1] == fr.kept(n_steps, rate) == c.lib.ofdm_conv_k7_kept_bits(n_steps, rate)
        wide = np.full((F, rows.shape[1] + 10), 99, np.int8)       # llr_stride > kept; the slack must not be read as LLRs
        wide[:, : rows.shape[1]] = rows
        dev = torch.from_numpy(wide).to(c.device)
        depunctured = np.zeros((F, 2 * n_steps), np.int64)
        depunctured[:, keep] = rows
        for term in (True, False):
            got = c.viterbi_decode_soft(dev, n_steps=n_steps, terminated=term, rate=rate)
            c.synchronize()
            assert got.shape == (F, n_steps // 8)
            np.testing.assert_array_equal(got.cpu().numpy(), cr.viterbi_batch(depunctured, term), err_msg=str((n_steps, rate, term)))
            if n_steps:
                assert c.last_dispatch() == "k_viterbi_k7f"
            assert not got[2 * (F // 4):3 * (F // 4)].any()           # both tie rules: all-zero LLRs decode to all-zero bytes
            if rate == 0:                                              # the existing entry point, byte for byte
                assert torch.equal(got, c.viterbi_decode_soft(dev, n_steps=n_steps, terminated=term))


def test_punctured_decoder_argument_checks():
    c = _ctx()
    llr = torch.zeros((2, 64), dtype=torch.int8, device=c.device)
    out = torch.zeros((2, 4), dtype=torch.uint8, device=c.device)
    f = c.lib.ofdm_conv_k7_decode_punctured
    assert f(c.h, llr.data_ptr(), 2, 47, 32, 1, 1, out.data_ptr(), 4) == -1       # llr_stride below kept(32, 2/3) = 48
    assert f(c.h, llr.data_ptr(), 2, 48, 32, 1, 1, out.data_ptr(), 4) == 0
    assert f(c.h, llr.data_ptr(), 2, 42, 32, 2, 1, out.data_ptr(), 4) == -1       # kept(32, 3/4) = 43
    assert f(c.h, llr.data_ptr(), 2, 43, 32, 2, 1, out.data_ptr(), 4) == 0
    assert f(c.h, llr.data_ptr(), 2, 64, 32, 1, 1, out.data_ptr(), 3) == -1       # out_stride below the row
    assert f(c.h, llr.data_ptr(), 2, 64, 32, 3, 1, out.data_ptr(), 4) == -1       # no such rate
    assert f(c.h, llr.data_ptr(), 2, 64, 32, -1, 1, out.data_ptr(), 4) == -1
    assert f(c.h, llr.data_ptr(), -1, 64, 32, 1, 1, out.data_ptr(), 4) == -1
    assert f(c.h, llr.data_ptr(), 2, 64, -1, 1, 1, out.data_ptr(), 4) == -1
    assert f(c.h, llr.data_ptr(), 1, 1 << 22, (1 << 20) + 1, 2, 1, out.data_ptr(), 1 << 18) == -2   # OFDM_ERR_UNSUPPORTED
    assert f(c.h, None, 0, 0, 0, 1, 1, None, 0) == 0 and f(c.h, None, 3, 0, 0, 2, 1, None, 0) == 0  # nothing to do, nothing written
    c.synchronize()


# ---------------------------------------------------------------------------------------------------------- 3. transmit
def _streams(pay, lens, rate, width):
    out = np.zeros((pay.shape[0], width), np.uint8)
    for f, ln in enumerate(lens):
        s = fr.encode_stream(pay[f, :ln].tobytes(), rate)
        out[f, : s.size] = s
    return out


@pytest.mark.parametrize("n,mod", [(64, 6), (1024, 4), (256, 1)])
def test_transmit_is_the_uncoded_frame_of_the_framed_stream(n, mod):
    api = _api()
    u = _ctx(n_fft=n, modulation=mod, ecc=api.ECC_NONE)
    for rate in RATES:
        c = _ctx(n_fft=n, modulation=mod, ecc=_framed(rate))
        for p in (0, 1, 560, 1304):
            assert c.coded_len(p) == fr.coded_len(p, rate)
            assert (c.data_symbols(p), c.frame_samples(p)) == (u.data_symbols(fr.coded_len(p, rate)), u.frame_samples(fr.coded_len(p, rate)))
        g = torch.Generator(device="cuda"); g.manual_seed(n + mod + rate)
        pay = torch.randint(0, 256, (5, 777), dtype=torch.uint8, device=c.device, generator=g)
        host = pay.cpu().numpy()
        width = fr.coded_len(777, rate)
        tx = c.encode_batch(pay)
        assert "k_conv_encode_p" in c.last_dispatch().split("+") and "k_conv_encode" not in c.last_dispatch().split("+")
        coded = torch.from_numpy(_streams(host, [777] * 5, rate, width)).to(c.device)
        assert torch.equal(tx, u.encode_batch(coded))
        lens = [777, 0, 13, 500, 776]
        coded = torch.from_numpy(_streams(host, lens, rate, width)).to(c.device)
        clen = torch.tensor([fr.coded_len(ln, rate) for ln in lens], dtype=torch.int32)
        assert torch.equal(c.encode_batch(pay, lens=torch.tensor(lens, dtype=torch.int32)), u.encode_batch(coded, lens=clen))


# ---------------------------------------------------------------------------------------------------------- helpers of 4-12
def _reference_decode(c, rx, r, max_symbols, rate):
    """per frame that reached the demodulator (status 0, or OFDM_FRAME_HEADER set behind it): (status, out_len, bytes) by the rule of
    the header -- framed_ref.decode_stream over the LLRs rx_llr returns for the frame, from LLR 128 on"""
    hk = c.estimate_channel(rx, r["offset"], r["f_delta"])
    L = c.rx_llr(rx, max_symbols, first_symbol=10, offset=r["offset"], f_delta=r["f_delta"], hk=hk)
    c.synchronize()
    L = L.cpu().numpy()
    body = max_symbols * c.bytes_per_symbol - 16
    want = {}
    for f in range(rx.shape[0]):
        if int(r["status"][f]) not in (0, fr.HEADER_STATUS):
            continue
        st, data = fr.decode_stream(L[f, 128:128 + 8 * body], body, rate)
        want[f] = (st, len(data), data)
    return want


# ---------------------------------------------------------------------------------------------------------- 4. chain = stages
@pytest.mark.parametrize("n,mod", [(64, 6), (256, 4), (1024, 6), (4096, 2)])
def test_chain_is_the_composition_of_the_stages(n, mod):
    for rate in RATES:
        c, pay, rx, D = _link(_framed(rate), n, mod, 7, 400, _data_snr(n, 16.0), 5 + n + rate)
        r = c.decode_batch(rx, max_symbols=D)
        c.synchronize()
        want = _reference_decode(c, rx, r, D, rate)
        assert sum(1 for st, _, _ in want.values() if st == 0) >= 5
        assert_rows_are(r, want)
        assert_rows_are(assert_chunking_changes_nothing(c, rx, D, r), want)   # many chunks of the LLR workspace


# ---------------------------------------------------------------------------------------------------------- 5. clean channel
@pytest.mark.parametrize("n", [64, 256, 1024, 4096])
def test_clean_channel_returns_the_payload(n):
    for rate in RATES:
        for i, (mod, guard) in enumerate(((1, True), (2, False), (4, True), (6, True), (8, False))):
            payload = 300 + 37 * i
            c, pay, rx, D = _link(_framed(rate), n, mod, 4, payload, _data_snr(n, 38.0 if mod == 8 else 30.0), 100 * n + 10 * rate + i, guard=guard)
            r = c.decode_batch(rx, max_symbols=D)
            c.synchronize()
            assert (r["status"] == 0).all() and (r["len"] == payload).all(), (n, rate, mod)
            assert torch.equal(r["bytes"][:, :payload], pay), (n, rate, mod)
        for payload in (0, 1):
            c, pay, rx, D = _link(_framed(rate), n, 6, 3, payload, _data_snr(n, 30.0), 7 * n + payload + rate)
            r = c.decode_batch(rx, max_symbols=D)
            c.synchronize()
            assert (r["status"] == 0).all() and (r["len"] == payload).all(), (n, rate, payload)
            assert torch.equal(r["bytes"][:, :payload], pay), (n, rate, payload)


# ---------------------------------------------------------------------------------------------------------- 6. a frame cut short
@pytest.mark.parametrize("n,mod", [(64, 6), (1024, 4)])
def test_cut_frame_delivers_the_unterminated_prefix(n, mod):
    for rate in RATES:
        c, pay, rx, D = _link(_framed(rate), n, mod, 4, 700, _data_snr(n, 30.0), 31 + n + rate)
        short = D - 2
        body = short * c.bytes_per_symbol - 16
        assert 18 < body < c.coded_len(700)
        T = fr.max_steps(8 * (body - 18), rate)
        n_out = min(700, T // 8)
        r = c.decode_batch(rx, max_symbols=short)
        c.synchronize()
        assert (r["status"] == 0).all() and (r["len"] == n_out).all()
        want = _reference_decode(c, rx, r, short, rate)
        assert len(want) == 4
        assert_rows_are(r, want)
        hk = c.estimate_channel(rx, r["offset"], r["f_delta"])
        L = c.rx_llr(rx, short, first_symbol=10, offset=r["offset"], f_delta=r["f_delta"], hk=hk).cpu().numpy()
        for f in range(4):   # spelled out: the unterminated reference over what is there of the body
            assert want[f][2] == bytes(fr.viterbi_punctured(L[f, 128 + 144:128 + 8 * body], T, rate, False)[:n_out])
            # a clean channel: what was received of the payload is right, except possibly the last bytes next to the open end
            assert want[f][2][: n_out - 8] == bytes(pay[f, : n_out - 8].cpu().numpy())


# ---------------------------------------------------------------------------------------------------------- 7. no valid length
def test_invalid_length_block_is_reported_not_guessed():
    api = _api()
    u = _ctx(ecc=api.ECC_NONE)
    rng = np.random.default_rng(70)
    pay = rng.integers(0, 256, 100, dtype=np.uint8).tobytes()
    for rate in RATES:
        c = _ctx(ecc=_framed(rate))
        good = fr.encode_stream(pay, rate)
        bad_head = cr.encode((100).to_bytes(4, "little") + (100 ^ 0xFFFFFFFE).to_bytes(4, "little"))   # a wrong complement, well coded
        bad_tail = cr.encode((100).to_bytes(4, "little") + (100 ^ 0xFFFFFFFF).to_bytes(4, "little") + b"\1")[:18]   # byte 8 is not 0
        rows = np.stack([good, np.concatenate([bad_head, good[18:]]), np.concatenate([bad_tail, good[18:]]), good])
        tx = u.encode_batch(torch.from_numpy(rows).to(u.device))
        rx = u.channel_batch(tx, snr_db=40.0, seed=7, span=tx.shape[1] + 160)
        D = c.data_symbols(100)
        assert D == u.data_symbols(rows.shape[1])
        for _ in range(2):                                  # deterministically
            r = c.decode_batch(rx, max_symbols=D)
            c.synchronize()
            assert r["status"].tolist() == [0, api.FRAME_HEADER, api.FRAME_HEADER, 0]
            assert r["len"].tolist() == [100, 0, 0, 100]
            for f in (0, 3):
                assert bytes(r["bytes"][f, :100].cpu().numpy()) == pay


def test_too_short_a_body_is_a_header_failure():
    api = _api()
    c, pay, rx, D = _link(api.ECC_CONV_K7F_R23, 64, api.BPSK, 3, 40, 30.0, 81)
    assert c.bytes_per_symbol == 6
    for syms, body in ((5, 14), (3, 2)):                    # 16 <= demodulated bytes < 16 + 18: a header, but no length block
        assert syms * c.bytes_per_symbol - 16 == body
        r = c.decode_batch(rx, max_symbols=syms)
        c.synchronize()
        assert (r["status"] == api.FRAME_HEADER).all() and (r["len"] == 0).all()
    r = c.decode_batch(rx, max_symbols=6)                   # body 20: the length block is there, the payload is cut to nothing much
    c.synchronize()
    assert (r["status"] == 0).all() and (r["len"] == fr.max_steps(8 * 2, 1) // 8).all()


# ---------------------------------------------------------------------------------------------------------- 8. entry points
def test_every_decode_entry_point_in_a_framed_mode():
    api = _api()
    ecc = api.ECC_CONV_K7F_R23
    c, pay, rx, D = _link(ecc, 64, 6, 6, 560, 16.0, 77)
    r, ones = assert_entry_points_agree(api, c, rx, D, dict(ecc=ecc))
    assert int((r["status"] == 0).sum()) >= 4
    for f, (st, n_out, _, _) in enumerate(ones):
        if st == 0:
            assert api.decode_long(rx[f].cpu().numpy(), True, api.QAM64, ecc=ecc)["len"] == n_out
    for e in (api.ECC_CONV_K7F_R12, api.ECC_CONV_K7F_R23, api.ECC_CONV_K7F_R34):
        assert api.decode(api.encode(b"a trellis of 64 states", True, api.QAM16, ecc=e), True, api.QAM16, ecc=e) == b"a trellis of 64 states"
    # a row too short for what the chain can write is refused; decode_batch's own rows are long enough
    need = fr.max_steps(8 * (D * c.bytes_per_symbol - 16 - 18), 1) // 8
    assert need <= D * c.bytes_per_symbol - 16
    assert_refuses_short_rows(c, rx, D, need)
    out = torch.zeros((1, 8), dtype=torch.uint8, device=c.device)
    i32 = torch.zeros((2,), dtype=torch.int32, device=c.device)
    # a max_symbols whose body could exceed 2^20 steps (rate 3/4: 6 steps per body byte) is refused before anything runs
    c34 = _ctx(ecc=api.ECC_CONV_K7F_R34)
    big = (1 << 20) // 6 // c34.bytes_per_symbol + 8
    assert c34.lib.ofdm_rx_decode_batch(c34.h, rx.data_ptr(), 1, rx.shape[1], rx.shape[1], 0, big, out.data_ptr(), big * c34.bytes_per_symbol,
                                        i32.data_ptr(), i32[1:].data_ptr(), None, None, None) == -2
    c.synchronize()


# ---------------------------------------------------------------------------------------------------------- 9. dispatch
@pytest.mark.parametrize("n", [64, 1024])
def test_dispatch_names_the_framed_kernels(n):
    api = _api()
    c, pay, rx, D = _link(api.ECC_CONV_K7F_R34, n, 6, 2, 300, 30.0, 3)
    c.decode_batch(rx, max_symbols=D)
    dc = c.last_dispatch()
    assert "k_sym<llr>" in dc and "k_viterbi_k7f" in dc and "k_rx_finish" not in dc, dc
    v, _, rxv, Dv = _link(api.ECC_CONV_K7, n, 6, 2, 300, 30.0, 3)         # the unframed mode keeps its kernels
    v.decode_batch(rxv, max_symbols=Dv)
    assert "k_viterbi_k7f" not in v.last_dispatch() and "k_viterbi_k7" in v.last_dispatch().split("+")
    v.encode_batch(pay)
    assert "k_conv_encode_p" not in v.last_dispatch() and "k_conv_encode" in v.last_dispatch().split("+")
    c.encode_batch(pay)
    assert "k_conv_encode_p" in c.last_dispatch().split("+")


# ---------------------------------------------------------------------------------------------------------- 10. the point of the feature
def test_coded_length_block_delivers_more_frames_than_the_uncoded_header():
    """N = 64, 64-QAM, guard bands, 12 dB: the same payloads, delays, CFO and channel seed for OFDM_ECC_CONV_K7 (length from the hard
    bits of the 16-byte header) and OFDM_ECC_CONV_K7F_R12 (length from the coded block).  The counts are printed (measured on an
    MI355X: 745 against 1 024 of 1 024 frames delivered whole, no framed frame with a wrong length); the record over 4 096 frames is
    profiles/framed_ber_and_speed.json."""
    api = _api()
    res = {}
    for ecc in (api.ECC_CONV_K7, api.ECC_CONV_K7F_R12):
        c, pay, rx, D = _link(ecc, 64, 6, 1024, 560, 12.0, 9012)
        r = c.decode_batch(rx, max_symbols=D)
        c.synchronize()
        res[ecc] = (r, pay, delivered(r, pay, 560)[0])
    assert torch.equal(res[api.ECC_CONV_K7][1], res[api.ECC_CONV_K7F_R12][1])          # the same payloads
    r = res[api.ECC_CONV_K7F_R12][0]
    n_old, n_new = int(res[api.ECC_CONV_K7][2].sum()), int(res[api.ECC_CONV_K7F_R12][2].sum())
    wrong_len = int(((r["status"] == 0) & (r["len"] != 560)).sum())
    print(f"12 dB, 1024 frames delivered whole: CONV_K7 {n_old}, CONV_K7F_R12 {n_new}; framed status 0 with a wrong length: {wrong_len}; "
          f"framed invalid length blocks: {int((r['status'] == api.FRAME_HEADER).sum())}")
    assert n_new > n_old, (n_new, n_old)
    assert wrong_len == 0
