"""GPU checks of the batched Reed-Solomon(255,223) kernels (k_rs255_encode, k_rs255_decode), their stage entry points and the
RS-outer frame modes OFDM_ECC_RS255 = 20 + inner.  The definition is the host code of ofdm_amd/csrc/outer_code.hip (pinned to the
oracle in tests/test_rs_modes_cpu.py), applied block by block; everything here is compared byte for byte, nothing has a tolerance."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rs_vectors as rv  # noqa: E402
from chain_checks import (assert_chunking_changes_nothing, assert_entry_points_agree, assert_refuses_short_rows, assert_rows_are,  # noqa: E402
                          ofdm_api as _api)
from chain_refs import rs_composition as _composition  # noqa: E402
from tools.link import data_snr as _data_snr, delivered, link as _link  # noqa: E402

pytestmark = pytest.mark.gpu

RS_MODES = (20, 30, 31, 32)
OLD_MODES = (0, 1, 2, 5, 10, 11, 12)
UNCORRECTABLE = -5


def _ctx(**kw):
    api = _api()
    kw.setdefault("n_fft", 64)
    kw.setdefault("modulation", api.QAM64)
    kw.setdefault("guard_bands", True)
    return api.Context(**kw)


@pytest.fixture(scope="module")
def stage():
    return _ctx(ecc=20)


def _strided(c, rows: np.ndarray, slack: int) -> torch.Tensor:
    """the rows on the device with a row stride `slack` bytes larger than the row (0xEE in between)"""
    n, nb = rows.shape
    big = torch.full((n, nb + slack), 0xEE, dtype=torch.uint8, device=c.device)
    big[:, :nb] = torch.from_numpy(np.ascontiguousarray(rows)).to(c.device)
    return big[:, :nb]


# ---------------------------------------------------------------------------------------------------------- 1. the encoder
@pytest.mark.parametrize("n_bytes", [0, 1, 222, 223, 224, 446, 560])
def test_encoder_is_the_host_encoder(stage, n_bytes):
    c = stage
    rng = np.random.default_rng(100 + n_bytes)
    data = rng.integers(0, 256, (5, n_bytes), dtype=np.uint8)
    full = 255 * (n_bytes // 223 + 1)
    dev = _strided(c, data, 9)
    for lens in (None, np.array([n_bytes, 0, n_bytes // 2, n_bytes + 5, -1], np.int32)):
        out = c.rs255_encode(dev, None if lens is None else torch.from_numpy(lens))
        c.synchronize()
        assert "k_rs255_encode" in c.last_dispatch()
        out = out.cpu().numpy()
        assert out.shape == (5, full)
        for f in range(5):
            ln = n_bytes if lens is None else rv.clamp(lens[f], n_bytes)
            want = rv.host_encode(c.lib, bytes(data[f, :ln]))
            assert bytes(out[f]) == want + bytes(full - len(want)), (n_bytes, f, ln)


# ---------------------------------------------------------------------------------------------------------- 2. the decoder
def _check_decoded(c, rows, lens, got, n_code):
    out, out_len, fixed = (t.cpu().numpy() for t in got)
    assert out.shape == (rv.ROWS, 223 * (n_code // 255 + 1))
    seen = set()
    for r in range(rv.ROWS):
        ln = n_code if lens is None else rv.clamp(lens[r], n_code)
        want, want_len, want_fixed = rv.host_row(c.lib, rows[r], ln)
        assert out_len[r] == want_len and fixed[r] == want_fixed, (n_code, r, ln, out_len[r], fixed[r], want_fixed)
        assert bytes(out[r, :want_len]) == want, (n_code, r, ln)
        seen.add("bad" if want_fixed < 0 else "fixed" if want_fixed else "clean")
    return seen, [bytes(out[r, :out_len[r]]) for r in range(rv.ROWS)], out_len.tolist(), fixed.tolist()


@pytest.mark.parametrize("n_code", rv.N_CODES)
def test_decoder_is_the_host_decoder(stage, n_code):
    c = stage
    rows = rv.decoder_rows(c.lib, n_code)
    dev = _strided(c, rows, 5)
    for lens in (None, rv.row_lengths(n_code)):
        tl = None if lens is None else torch.from_numpy(lens)
        got = c.rs255_decode(dev, tl)
        c.synchronize()
        assert "k_rs255_decode" in c.last_dispatch()
        base = _check_decoded(c, rows, lens, got, n_code)
        if lens is None and n_code >= 255:                  # rows of every outcome (one-block rows: a wholly clean one too)
            assert base[0] >= {"bad", "fixed"} and (n_code != 255 or "clean" in base[0]), base[0]
        for cap in (1, 3):                                  # many rows per wavefront, the grid not a divisor of the rows
            c.set_tuning("grid_cap", cap)
            try:
                again = c.rs255_decode(dev, tl)
                c.synchronize()
            finally:
                c.set_tuning("grid_cap", 0)
            assert _check_decoded(c, rows, lens, again, n_code)[1:] == base[1:], (n_code, cap)


# ---------------------------------------------------------------------------------------------------------- 3. argument checks
def test_stage_argument_checks(stage):
    c = stage
    enc, dec = c.lib.ofdm_rs255_encode_batch, c.lib.ofdm_rs255_decode_batch
    buf = torch.full((4096,), 0x5A, dtype=torch.uint8, device=c.device)
    i32 = torch.zeros((8,), dtype=torch.int32, device=c.device)
    p = buf.data_ptr()
    assert enc(c.h, p, 2, 300, None, 300, p + 1024, 510) == 0
    assert enc(c.h, p, 2, 299, None, 300, p + 1024, 510) == -1          # in_stride < n_bytes
    assert enc(c.h, p, 2, 300, None, 300, p + 1024, 509) == -1          # out_stride < encoded_len
    assert enc(c.h, p, -1, 300, None, 300, p + 1024, 510) == -1
    assert enc(c.h, p, 2, 300, None, -1, p + 1024, 510) == -1
    assert dec(c.h, p, 2, 300, None, 300, p + 1024, 446, i32.data_ptr(), i32[4:].data_ptr()) == 0
    assert dec(c.h, p, 2, 299, None, 300, p + 1024, 446, None, None) == -1   # code_stride < n_code
    assert dec(c.h, p, 2, 300, None, 300, p + 1024, 445, None, None) == -1   # out_stride < decoded_len
    assert dec(c.h, p, -1, 300, None, 300, p + 1024, 446, None, None) == -1
    assert dec(c.h, p, 2, 300, None, -1, p + 1024, 446, None, None) == -1
    c.synchronize()
    # n_frames = 0: OFDM_OK and nothing written
    mark = torch.full((1024,), 0xC3, dtype=torch.uint8, device=c.device)
    assert enc(c.h, p, 0, 300, None, 300, mark.data_ptr(), 510) == 0
    assert dec(c.h, p, 0, 300, None, 300, mark.data_ptr(), 446, None, None) == 0
    c.synchronize()
    assert bool((mark == 0xC3).all())


# ---------------------------------------------------------------------------------------------------------- 4. transmit
@pytest.mark.parametrize("n,mod", [(64, 6), (1024, 4)])
def test_transmit_is_the_inner_frame_of_the_rs_coded_payload(n, mod):
    api = _api()
    rng = np.random.default_rng(n)
    p = 300
    full = 255 * (p // 223 + 1)
    pay = rng.integers(0, 256, (4, p), dtype=np.uint8)
    for ecc in RS_MODES:
        c, inner = _ctx(n_fft=n, modulation=mod, ecc=ecc), _ctx(n_fft=n, modulation=mod, ecc=ecc - 20)
        for q in (0, 1, 222, 223, 560, 1304):
            coded = 255 * (q // 223 + 1)
            assert c.coded_len(q) == inner.coded_len(coded), (ecc, q)
            D = -(-(-(-((16 + c.coded_len(q)) * 8) // mod)) // c.data_carriers)
            assert c.data_symbols(q) == inner.data_symbols(coded) == D, (ecc, q)
            assert c.frame_samples(q) == inner.frame_samples(coded) == (10 + D) * c.S, (ecc, q)
        for lens in (None, np.array([p, 0, 223, 100], np.int32)):
            coded = np.zeros((4, full), np.uint8)
            clen = np.zeros(4, np.int32)
            for f in range(4):
                ln = p if lens is None else int(lens[f])
                cw = np.frombuffer(rv.host_encode(c.lib, bytes(pay[f, :ln])), np.uint8)
                coded[f, :cw.size], clen[f] = cw, cw.size
            got = c.encode_batch(c.to_device(pay), lens=None if lens is None else torch.from_numpy(lens))
            assert "k_rs255_encode" in c.last_dispatch()
            want = inner.encode_batch(inner.to_device(coded), lens=None if lens is None else torch.from_numpy(clen))
            c.synchronize(); inner.synchronize()
            assert got.shape == want.shape and torch.equal(got, want), (n, ecc, lens is None)


# ---------------------------------------------------------------------------------------------------------- 5. chain = composition
def _assert_is_composition(r, ri, want):
    assert_rows_are(r, dict(enumerate(want)))
    for k in ("offset", "f_delta", "metric"):
        assert torch.equal(r[k], ri[k]), k


@pytest.mark.parametrize("n", [64, 1024])
@pytest.mark.parametrize("ecc", [20, 31])
def test_chain_is_the_composition(n, ecc):
    c, pay, rx, D = _link(ecc, n, 6, 7, 560, _data_snr(n, 16.0), 5 + n)
    r = c.decode_batch(rx, max_symbols=D)
    c.synchronize()
    ri, want = _composition(c, rx, D)
    _assert_is_composition(r, ri, want)
    _assert_is_composition(assert_chunking_changes_nothing(c, rx, D, r), ri, want)


# ---------------------------------------------------------------------------------------------------------- 6. clean channel
@pytest.mark.parametrize("n", [64, 256, 1024])
def test_clean_channel_returns_the_padded_payload(n):
    for ecc in RS_MODES:
        for p in (0, 1, 223, 560):
            c, pay, rx, D = _link(ecc, n, 6, 3, p, _data_snr(n, 30.0), 11 * n + ecc + p)
            r = c.decode_batch(rx, max_symbols=D)
            c.synchronize()
            want_len = 223 * (255 * (p // 223 + 1) // 255 + 1)
            assert (r["status"] == 0).all() and (r["len"] == want_len).all(), (n, ecc, p, r["status"].tolist(), r["len"].tolist())
            assert torch.equal(r["bytes"][:, :p], pay), (n, ecc, p)
            assert not bool(r["bytes"][:, p:want_len].any()), (n, ecc, p)


# ---------------------------------------------------------------------------------------------------------- 7. a frame cut short
@pytest.mark.parametrize("ecc", [20, 31])
def test_cut_frame_is_uncorrectable(ecc):
    c, pay, rx, D = _link(ecc, 64, 6, 4, 560, 30.0, 31 + ecc)
    short = D - 2
    r = c.decode_batch(rx, max_symbols=short)
    c.synchronize()
    ri, want = _composition(c, rx, short)
    _assert_is_composition(r, ri, want)
    status, ln = r["status"].cpu().numpy(), r["len"].cpu().numpy()
    assert ((status == UNCORRECTABLE) & (ln == 0)).any(), (status, ln)


# ---------------------------------------------------------------------------------------------------------- 8. entry points
def test_every_decode_entry_point_in_rs_mode():
    api = _api()
    ecc = api.ECC_RS255_K7F_R34
    c, pay, rx, D = _link(ecc, 64, 6, 6, 560, 16.0, 77)
    assert_entry_points_agree(api, c, rx, D, dict(ecc=ecc))
    msg = b"sixteen bytes a block, and the block knows"
    rt = api.decode(api.encode(msg, True, api.QAM16, ecc=ecc), True, api.QAM16, ecc=ecc)
    assert rt == msg + bytes(2 * 223 - len(msg))               # decipher_transmission_bytes: whole blocks, the trailing zero block too
    # a row one byte too short for what the chain can write is refused
    body = D * c.bytes_per_symbol - 16
    bits = 8 * (body - 18)                                     # rate 3/4: the largest T with kept(T) <= bits (framed_ref.max_steps)
    T = 3 * (bits >> 2) + {0: 0, 1: 0, 2: 1, 3: 2}[bits & 3]
    assert c.lib.ofdm_conv_k7_kept_bits(T, 2) <= bits < c.lib.ofdm_conv_k7_kept_bits(T + 1, 2)
    need = 223 * ((T // 8) // 255 + 1)
    assert_refuses_short_rows(c, rx, D, need, accepts=True)     # ... and one of `need` bytes is taken


# ---------------------------------------------------------------------------------------------------------- 9. dispatch
def test_dispatch_names_the_rs_kernels():
    for n in (64, 1024):
        c, pay, rx, D = _link(20, n, 6, 2, 300, _data_snr(n, 30.0), 3)
        for ecc in RS_MODES + OLD_MODES:
            x = c if ecc == 20 else _ctx(n_fft=n, ecc=ecc)
            x.decode_batch(rx, max_symbols=D)
            x.synchronize()
            assert ("k_rs255_decode" in x.last_dispatch()) == (ecc in RS_MODES), (n, ecc, x.last_dispatch())
            assert "k_rs255_encode" not in x.last_dispatch()
            x.encode_batch(pay)
            x.synchronize()
            assert ("k_rs255_encode" in x.last_dispatch()) == (ecc in RS_MODES), (n, ecc, x.last_dispatch())
            assert "k_rs255_decode" not in x.last_dispatch()
        c.decode_batch(rx, max_symbols=D)                       # inner = NONE keeps the fused frame kernel, finish included
        assert ("k_rxframe%d<finish>" % n) in c.last_dispatch(), c.last_dispatch()


# ---------------------------------------------------------------------------------------------------------- 10. the code earns its keep
# N = 64, 64-QAM, guard bands, payload 560, 256 frames, seed 9012, the same payloads in both modes.  Conditions set before the run:
# rate 3/4 alone fails at least 30 frames; RS around it fails at most a quarter as many; no RS-mode frame is delivered wrong with
# status 0.  Operating point: 12 dB first (the issue's CPU simulation: 124 against 1), moved by whole dB only if the inner mode's
# count -- the parent's behaviour -- is outside 30 .. 200 there.
# Seen on an MI355X (frames of 256 not delivered right, rate 3/4 alone / RS around it / RS wrong with status 0): 12 dB 42 / 1 / 0, so
# 12 dB stands (42 is inside 30 .. 200); its neighbours 11 dB 87 / 1 / 0 and 13 dB 18 / 0 / 0.  The same counts are in
# profiles/rs_ber_and_speed.json ("test_rs_outer_code_earns_its_keep").
KEEP_SNR, KEEP_SEED = 12.0, 9012


def _not_delivered(api, ecc, snr):
    c, pay, rx, D = _link(ecc, 64, 6, 256, 560, snr, KEEP_SEED)
    r = c.decode_batch(rx, max_symbols=D)
    c.synchronize()
    right, ok = delivered(r, pay, 560 if ecc < 20 else 223 * 4)
    return pay, int((~right).sum()), int((ok & ~right).sum())


def test_rs_outer_code_earns_its_keep():
    api = _api()
    pay_i, bad_inner, _ = _not_delivered(api, api.ECC_CONV_K7F_R34, KEEP_SNR)
    pay_r, bad_rs, wrong_ok = _not_delivered(api, api.ECC_RS255_K7F_R34, KEEP_SNR)
    print(f"snr {KEEP_SNR}: rate 3/4 alone fails {bad_inner} of 256 frames, RS + rate 3/4 fails {bad_rs}, {wrong_ok} wrong with status 0")
    assert torch.equal(pay_i, pay_r)
    assert bad_inner >= 30, bad_inner
    assert 4 * bad_rs <= bad_inner, (bad_rs, bad_inner)
    assert wrong_ok == 0, wrong_ok
