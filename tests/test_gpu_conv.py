"""GPU checks of the convolutional mode (OFDM_ECC_CONV_K7: k_conv_encode, k_viterbi_k7 and the decode chain around them) against
the numpy restatement tests/conv_ref.py.  Everything compared with conv_ref is compared bit for bit: once the LLRs exist nothing
here is floating point, so no comparison in this file has a tolerance."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_ref as cr  # noqa: E402
from chain_checks import (assert_chunking_changes_nothing, assert_entry_points_agree, assert_refuses_short_rows, assert_rows_are,  # noqa: E402
                          ofdm_api as _api)
from chain_refs import conv_reference_decode, decoder_rows as _decoder_rows  # noqa: E402
from tools.link import bit_errors, data_snr as _data_snr, link as _link  # noqa: E402

pytestmark = pytest.mark.gpu

MODS = (1, 2, 4, 6, 8)
KNOWN = (("", "0000"), ("61", "fb689c03"), ("616263", "fb68708c8bb89c03"), ("0001020304050607", "0000fb34ecd317e7b04f487b5f9ca4a80300"))


def _ctx(**kw):
    api = _api()
    kw.setdefault("n_fft", 64)
    kw.setdefault("modulation", api.QAM64)
    kw.setdefault("guard_bands", True)
    kw.setdefault("ecc", api.ECC_CONV_K7)
    return api.Context(**kw)


# ---------------------------------------------------------------------------------------------------------- 5. the encoder stage
def test_encoder_known_answers():
    c = _ctx()
    for pay, code in KNOWN:
        src = torch.from_numpy(np.frombuffer(bytes.fromhex(pay), np.uint8).copy()).to(c.device).reshape(1, -1)
        got = c.conv_encode(src)
        c.synchronize()
        assert bytes(got[0].cpu().numpy()).hex() == code
    assert c.last_dispatch() == "k_conv_encode"


@pytest.mark.parametrize("n_bytes", [0, 1, 2, 3, 63, 64, 560, 1304])
def test_encoder_matches_the_restatement(n_bytes):
    c = _ctx()
    rng = np.random.default_rng(100 + n_bytes)
    F = 5
    wide = rng.integers(0, 256, (F, n_bytes + 7), dtype=np.uint8)
    dev = torch.from_numpy(wide).to(c.device)
    got = c.conv_encode(dev[:, :n_bytes])                      # a row stride larger than the row
    c.synchronize()
    assert got.shape == (F, 2 * (n_bytes + 1))
    for f in range(F):
        np.testing.assert_array_equal(got[f].cpu().numpy(), cr.encode(wide[f, :n_bytes].tobytes()))
    assert c.lib.ofdm_conv_k7_encode(c.h, dev.data_ptr(), F, n_bytes - 1, n_bytes, got.data_ptr(), got.shape[1]) == -1
    assert c.lib.ofdm_conv_k7_encode(c.h, dev.data_ptr(), F, n_bytes + 7, n_bytes, got.data_ptr(), got.shape[1] - 1) == -1


# ---------------------------------------------------------------------------------------------------------- 6. the decoder stage
@pytest.mark.parametrize("n_steps", [0, 8, 13, 48, 64, 65, 1000, 4488, 10440])
def test_decoder_matches_the_restatement(n_steps):
    c = _ctx()
    c.set_tuning("grid_cap", 2)                                   # 8 wavefronts: every one of them decodes several frames
    rng = np.random.default_rng(200 + n_steps)
    rows, sent = _decoder_rows(rng, n_steps, 10 if n_steps < 4000 else 6)
    F = rows.shape[0]
    wide = np.full((F, 2 * n_steps + 10), 99, np.int8)            # llr_stride > 2 n_steps; the slack must not be read as LLRs
    wide[:, : 2 * n_steps] = rows
    dev = torch.from_numpy(wide).to(c.device)
    for term in (True, False):
        got = c.viterbi_decode_soft(dev, n_steps=n_steps, terminated=term)
        c.synchronize()
        assert got.shape == (F, n_steps // 8)
        np.testing.assert_array_equal(got.cpu().numpy(), cr.viterbi_batch(rows, term), err_msg=str((n_steps, term)))
        if n_steps:
            assert c.last_dispatch() == "k_viterbi_k7"
        assert not got[2 * (F // 4):3 * (F // 4)].any()           # both tie rules: all-zero LLRs decode to all-zero bytes
        np.testing.assert_array_equal(got[3 * (F // 4):].cpu().numpy(), sent)    # a codeword at full confidence: its own input
    if n_steps >= 8:   # n_steps defaults to what the rows hold
        np.testing.assert_array_equal(c.viterbi_decode_soft(dev[:, : 2 * n_steps], terminated=False).cpu().numpy(), got.cpu().numpy())


def test_decoder_argument_checks():
    c = _ctx()
    llr = torch.zeros((2, 64), dtype=torch.int8, device=c.device)
    out = torch.zeros((2, 4), dtype=torch.uint8, device=c.device)
    f = c.lib.ofdm_conv_k7_decode_soft
    assert f(c.h, llr.data_ptr(), 2, 63, 32, 1, out.data_ptr(), 4) == -1          # llr_stride below the row
    assert f(c.h, llr.data_ptr(), 2, 64, 32, 1, out.data_ptr(), 3) == -1          # out_stride below the row
    assert f(c.h, llr.data_ptr(), -1, 64, 32, 1, out.data_ptr(), 4) == -1
    assert f(c.h, llr.data_ptr(), 2, 64, -1, 1, out.data_ptr(), 4) == -1
    assert f(c.h, llr.data_ptr(), 1, 1 << 22, (1 << 20) + 1, 1, out.data_ptr(), 1 << 18) == -2   # OFDM_ERR_UNSUPPORTED
    assert f(c.h, None, 0, 0, 0, 1, None, 0) == 0 and f(c.h, None, 3, 0, 0, 1, None, 0) == 0      # nothing to do, nothing written


# ---------------------------------------------------------------------------------------------------------- 7. transmit
@pytest.mark.parametrize("n,mod", [(64, 6), (1024, 4), (256, 1)])
def test_transmit_is_the_uncoded_frame_of_the_coded_bytes(n, mod):
    api = _api()
    c = _ctx(n_fft=n, modulation=mod)
    u = _ctx(n_fft=n, modulation=mod, ecc=api.ECC_NONE)
    for p in (0, 1, 560, 1304):
        assert c.coded_len(p) == 2 * (p + 1)
        assert (c.data_symbols(p), c.frame_samples(p)) == (u.data_symbols(2 * (p + 1)), u.frame_samples(2 * (p + 1)))
    g = torch.Generator(device="cuda"); g.manual_seed(n + mod)
    pay = torch.randint(0, 256, (5, 777), dtype=torch.uint8, device=c.device, generator=g)
    tx = c.encode_batch(pay)
    assert "k_conv_encode" in c.last_dispatch()
    assert torch.equal(tx, u.encode_batch(c.conv_encode(pay)))
    lens = torch.tensor([777, 0, 13, 500, 776], dtype=torch.int32)
    coded = torch.zeros((5, 2 * 778), dtype=torch.uint8, device=c.device)
    for f, ln in enumerate(lens.tolist()):
        coded[f, : 2 * (ln + 1)] = c.conv_encode(pay[f:f + 1, :ln].contiguous())[0]
    assert torch.equal(c.encode_batch(pay, lens=lens), u.encode_batch(coded, lens=2 * (lens + 1)))


# ---------------------------------------------------------------------------------------------------------- helpers of 8-13
def _reference_decode(c, rx, r, max_symbols):
    """chain_refs.conv_reference_decode as {frame: (status 0, out_len, bytes)}"""
    return {f: (0, n_out, data) for f, (n_out, data) in conv_reference_decode(c, rx, r, max_symbols).items()}


# ---------------------------------------------------------------------------------------------------------- 8. chain = stages
@pytest.mark.parametrize("n,mod", [(64, 6), (256, 4), (1024, 6), (4096, 2)])
def test_chain_is_the_composition_of_the_stages(n, mod):
    api = _api()
    c, pay, rx, D = _link(api.ECC_CONV_K7, n, mod, 7, 400, _data_snr(n, 16.0), 5 + n)
    r = c.decode_batch(rx, max_symbols=D)
    c.synchronize()
    want = _reference_decode(c, rx, r, D)
    assert len(want) >= 5
    assert_rows_are(r, want)
    assert_rows_are(assert_chunking_changes_nothing(c, rx, D, r), want)   # many chunks of the LLR workspace


# ---------------------------------------------------------------------------------------------------------- 9. a frame cut short
@pytest.mark.parametrize("n,mod", [(64, 6), (1024, 4)])
def test_cut_frame_is_decoded_unterminated(n, mod):
    api = _api()
    c, pay, rx, D = _link(api.ECC_CONV_K7, n, mod, 4, 700, _data_snr(n, 30.0), 31 + n)
    short = D - 2
    body = short * c.bytes_per_symbol - 16
    assert 0 < body < c.coded_len(700)
    r = c.decode_batch(rx, max_symbols=short)
    c.synchronize()
    assert (r["status"] == 0).all()
    assert (r["len"] == body // 2 - 1).all()
    want = _reference_decode(c, rx, r, short)
    assert_rows_are(r, want)
    hk = c.estimate_channel(rx, r["offset"], r["f_delta"])
    L = c.rx_llr(rx, short, first_symbol=10, offset=r["offset"], f_delta=r["f_delta"], hk=hk).cpu().numpy()
    for f in range(4):   # spelled out: the unterminated reference over the whole cut body
        assert want[f][2] == bytes(cr.viterbi(L[f, 128:128 + 8 * body], terminated=False)[: body // 2 - 1])
        # a clean channel: what was received of the payload is right, except possibly the last bytes next to the open end
        assert want[f][2][: body // 2 - 8] == bytes(pay[f, : body // 2 - 8].cpu().numpy())


# ---------------------------------------------------------------------------------------------------------- 10. clean channel
@pytest.mark.parametrize("n", [64, 256, 1024, 4096])
def test_clean_channel_returns_the_payload(n):
    api = _api()
    for guard in (True, False):
        for i, mod in enumerate(MODS):
            payload = 300 + 37 * i
            # the SNRs of test_gpu_soft.py::test_clean_channel_soft_equals_hard (256-QAM: 38 dB, for its uncoded length header)
            c, pay, rx, D = _link(api.ECC_CONV_K7, n, mod, 4, payload, _data_snr(n, 38.0 if mod == 8 else 30.0), 100 * n + i + (0 if guard else 50),
                                  guard=guard)
            r = c.decode_batch(rx, max_symbols=D)
            c.synchronize()
            assert (r["status"] == 0).all() and (r["len"] == payload).all(), (n, guard, mod)
            assert torch.equal(r["bytes"][:, :payload], pay), (n, guard, mod)
    for payload in (0, 1):
        c, pay, rx, D = _link(api.ECC_CONV_K7, n, 6, 3, payload, _data_snr(n, 30.0), 7 * n + payload)
        r = c.decode_batch(rx, max_symbols=D)
        c.synchronize()
        assert (r["status"] == 0).all() and (r["len"] == payload).all(), (n, payload)
        assert torch.equal(r["bytes"][:, :payload], pay), (n, payload)


# ---------------------------------------------------------------------------------------------------------- 11. entry points
def test_every_decode_entry_point_in_conv_mode():
    api = _api()
    c, pay, rx, D = _link(api.ECC_CONV_K7, 64, 6, 6, 560, 16.0, 77)
    assert_entry_points_agree(api, c, rx, D, dict(ecc=api.ECC_CONV_K7))
    rt = api.decode(api.encode(b"a trellis of 64 states", True, api.QAM16, ecc=api.ECC_CONV_K7), True, api.QAM16, ecc=api.ECC_CONV_K7)
    assert rt == b"a trellis of 64 states"
    # a row too short for what the chain can write is refused
    assert_refuses_short_rows(c, rx, D, (D * c.bytes_per_symbol - 16) // 2 - 1)


# ---------------------------------------------------------------------------------------------------------- 12. dispatch
@pytest.mark.parametrize("n", [64, 1024])
def test_dispatch_names_the_conv_kernels(n):
    api = _api()
    c, pay, rx, D = _link(api.ECC_CONV_K7, n, 6, 2, 300, 30.0, 3)
    c.decode_batch(rx, max_symbols=D)
    dc = c.last_dispatch()
    assert "k_sym<llr>" in dc and "k_viterbi_k7" in dc and "k_rx_finish" not in dc, dc
    s = api.Context(n_fft=n, modulation=6, guard_bands=True, ecc=api.ECC_HAMMING74_SOFT)
    s.decode_batch(rx, max_symbols=D)
    assert "k_viterbi_k7" not in s.last_dispatch() and "k_conv_encode" not in s.last_dispatch()
    s.encode_batch(pay)
    assert "k_conv_encode" not in s.last_dispatch()


# ---------------------------------------------------------------------------------------------------------- 13. the code earns its keep
# The two operating points of test_gpu_soft.py::test_soft_beats_hard_at_low_snr at which the committed curve
# (profiles/soft_ber_and_speed.json, N = 64, 4096 frames) leaves soft Hamming 4819 (12 dB) and 1384 (14 dB) payload bit errors.
# Conditions, from that curve alone: it decodes 2787 / 4096 and 3721 / 4096 headers there, and the header is the same uncoded 16
# bytes in both modes, so 1024 frames leave about 474 and 845 frames that both modes decode (three standard deviations below 474 is
# 426) with about 700 and 300 soft-Hamming bit errors among them.
CONV_POINTS = ((12.0, 9012), (14.0, 9014))


def _payload_bit_errors(r, pay, ok):
    return bit_errors(torch.bitwise_xor(r["bytes"][:, :pay.shape[1]], pay)[ok])


def test_conv_beats_soft_hamming_at_low_snr():
    api = _api()
    for snr, seed in CONV_POINTS:
        res = {}
        for ecc in (api.ECC_HAMMING74_SOFT, api.ECC_CONV_K7):
            c, pay, rx, D = _link(ecc, 64, 6, 1024, 560, snr, seed)
            r = c.decode_batch(rx, max_symbols=D)
            c.synchronize()
            res[ecc] = (r, pay, (r["status"] == 0) & (r["len"] == 560))
        assert torch.equal(res[api.ECC_HAMMING74_SOFT][1], res[api.ECC_CONV_K7][1])     # the same payloads
        both = res[api.ECC_HAMMING74_SOFT][2] & res[api.ECC_CONV_K7][2]
        e_ham = _payload_bit_errors(*res[api.ECC_HAMMING74_SOFT][:2], both)
        e_conv = _payload_bit_errors(*res[api.ECC_CONV_K7][:2], both)
        print(f"snr {snr}: common frames {int(both.sum())}, soft Hamming errors {e_ham}, conv errors {e_conv}")
        assert int(both.sum()) >= 400, (snr, int(both.sum()))
        assert e_ham >= 100, (snr, e_ham)
        assert e_conv < e_ham, (snr, e_conv, e_ham)
