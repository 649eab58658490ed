"""GPU checks of the CRC-32 frame check: the kernels k_fcs_wrap / k_fcs_check, their stage entry points and the frame modes
ecc = OFDM_ECC_FCS + mode.  The definition is tests/fcs_ref.py over zlib.crc32; everything here is compared byte for byte, nothing
has a tolerance."""
import functools
import os
import struct
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fcs_ref  # noqa: E402
from chain_checks import assert_entry_points_agree, assert_refuses_short_rows, ofdm_api as _api  # noqa: E402
from tools.link import delivered, generator, link_on, seeded_channel  # noqa: E402

pytestmark = pytest.mark.gpu

FCS = fcs_ref.ECC_FCS
FRAME_FCS, NOSYNC, UNCORRECTABLE = -6, -2, -5
SENTINEL = 0xEE


@functools.lru_cache(maxsize=None)
def _ctx(ecc=0, n_fft=64):
    api = _api()
    return api.Context(n_fft=n_fft, modulation=api.QAM64, guard_bands=True, ecc=ecc)


@pytest.fixture(scope="module")
def stage():
    return _ctx(0)                                               # the stage entry points work on any context, whatever its ecc


@pytest.fixture(scope="module")
def bitserial():
    """a context of its own whose k_fcs_wrap / k_fcs_check reduce every lane's chunk bit by bit in registers (laboratory key
    fcs_bitserial) instead of through the slice-by-4 tables in LDS"""
    api = _api()
    c = api.Context(n_fft=64, modulation=api.QAM64, guard_bands=True, tuning={"fcs_bitserial": 1})
    assert c.get_tuning("fcs_bitserial") == 1
    return c


def _embed(c, rows: np.ndarray, slack: int = 9):
    """the rows on the device at an ODD base address, the row stride `slack` bytes larger than the row, 0xEE everywhere else:
    (view [n, nb], the whole allocation)"""
    n, nb = rows.shape
    stride = nb + slack
    flat = torch.full((16 + n * stride + 16,), SENTINEL, dtype=torch.uint8, device=c.device)
    base = 1 if flat.data_ptr() % 2 == 0 else 2
    view = flat[base:base + n * stride].view(n, stride)[:, :nb]
    if nb:
        view.copy_(torch.from_numpy(np.ascontiguousarray(rows)).to(c.device))
    assert nb == 0 or view.data_ptr() % 2 == 1
    return view, flat


def _only_view_written(flat, view, n, nb, slack=9):
    """every byte of the allocation outside the [n, nb] view still holds the sentinel"""
    stride = nb + slack
    base = view.data_ptr() - flat.data_ptr() if nb else (1 if flat.data_ptr() % 2 == 0 else 2)
    host = flat.cpu().numpy()
    body = host[base:base + n * stride].reshape(n, stride)
    return bool((host[:base] == SENTINEL).all() and (host[base + n * stride:] == SENTINEL).all() and (body[:, nb:] == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------- 1. wrap is zlib
def _wrap_case(c, data: np.ndarray, lens):
    n, nb = data.shape
    src, _ = _embed(c, data)
    out, flat = _embed(c, np.zeros((n, nb + 8), np.uint8))
    out.fill_(SENTINEL)
    got, got_len = c.fcs_wrap(src, None if lens is None else torch.from_numpy(lens), want_len=True, out=out)
    c.synchronize()
    assert c.last_dispatch() == "k_fcs_wrap"
    host, host_len = got.cpu().numpy(), got_len.cpu().numpy()
    for f in range(n):
        ln = nb if lens is None else fcs_ref.clamp(lens[f], nb)
        want = fcs_ref.wrap(bytes(data[f, :ln]))
        assert host_len[f] == ln + 8, (nb, f, ln)
        assert bytes(host[f]) == want + bytes(nb + 8 - len(want)), (nb, f, ln)   # zeros behind a ragged envelope
    assert _only_view_written(flat, out, n, nb + 8), nb
    return host


WRAP_SIZES = [0, 1, 2, 3, 4, 5, 7, 8, 59, 60, 61, 63, 64, 65, 251, 252, 253, 255, 256, 257, 560, 1304, 4099]


@pytest.mark.parametrize("n_bytes", WRAP_SIZES)
def test_wrap_is_zlib(stage, n_bytes):
    rng = np.random.default_rng(1000 + n_bytes)
    data = rng.integers(0, 256, (7, n_bytes), dtype=np.uint8)
    _wrap_case(stage, data, None)
    _wrap_case(stage, data, np.array([n_bytes, 0, n_bytes // 2, n_bytes + 5, -1, min(n_bytes, 1), max(n_bytes - 1, 0)], np.int32))


def test_wrap_long_rows(stage):
    rng = np.random.default_rng(70001)
    data = rng.integers(0, 256, (4, 70001), dtype=np.uint8)
    _wrap_case(stage, data, None)
    _wrap_case(stage, data, np.array([70001, 0, 35000, 69999], np.int32))


def test_wrap_many_rows_per_wavefront(stage):
    c = stage
    rng = np.random.default_rng(300)
    data = rng.integers(0, 256, (300, 1304), dtype=np.uint8)
    lens = rng.integers(-3, 1310, 300).astype(np.int32)
    base = _wrap_case(c, data, lens)
    for cap in (1, 3):
        c.set_tuning("grid_cap", cap)
        try:
            again = _wrap_case(c, data, lens)
        finally:
            c.set_tuning("grid_cap", 0)
        assert np.array_equal(again, base), cap


# ---------------------------------------------------------------------------------------------------------- 2. check is the rule
def _forge(row: bytes, p: int, fix_crc: bool) -> bytes:
    out = bytearray(struct.pack("<I", p) + row[4:])
    if fix_crc and 8 + p <= len(out):
        struct.pack_into("<I", out, 4 + p, zlib.crc32(bytes(out[:4 + p])) & 0xFFFFFFFF)
    return bytes(out)


@functools.lru_cache(maxsize=None)
def _check_rows():
    rng = np.random.default_rng(2024)
    rnd = lambda n: bytes(rng.integers(0, 256, n, dtype=np.uint8))  # noqa: E731
    rows = []
    for p in (0, 1, 5, 32, 223, 560):
        env = fcs_ref.wrap(rnd(p))
        for pad in (0, 3, 223):
            rows += [env + bytes(pad), env + rnd(pad)]
        bad = bytearray(env + rnd(3))
        bad[len(env) // 2] ^= 0x10
        rows.append(bytes(bad))
    env40 = fcs_ref.wrap(rnd(32))
    for bit in range(320):                                       # every single-bit variant of one 40-byte envelope
        bad = bytearray(env40 + bytes(700))
        bad[bit >> 3] ^= 1 << (bit & 7)
        rows.append(bytes(bad))
    L = 64
    body = rnd(L)
    rows += [_forge(body, L - 7, True), _forge(body, L - 8, True), _forge(body, L - 8, False), _forge(body, 2 ** 31, True),
             _forge(body, 0xFFFFFFFF, True), _forge(body, 0, True), _forge(body, 0, False)]
    for length in range(10):
        rows += [fcs_ref.wrap(b"")[:length], fcs_ref.wrap(b"x")[:length], bytes(length), rnd(length)]
    return rows


def _check_case(c, rows, use_lens=True):
    n, n_row = len(rows), max(len(r) for r in rows)
    mat = np.full((n, n_row), SENTINEL, np.uint8)                # (bytes behind a row's own L_f are not zeros)
    lens = np.zeros(n, np.int32)
    for f, r in enumerate(rows):
        mat[f, :len(r)] = np.frombuffer(r, np.uint8)
        lens[f] = len(r)
    src, _ = _embed(c, mat)
    out, flat = _embed(c, np.zeros((n, max(n_row - 8, 0)), np.uint8))
    out.fill_(SENTINEL)
    got, got_len, ok = c.fcs_check(src, torch.from_numpy(lens) if use_lens else None, out=out)
    c.synchronize()
    assert c.last_dispatch() == "k_fcs_check"
    got, got_len, ok = got.cpu().numpy(), got_len.cpu().numpy(), ok.cpu().numpy()
    verdicts = []
    for f, r in enumerate(rows):
        want = fcs_ref.check(r if use_lens else bytes(mat[f]))
        if want is None:
            assert (ok[f], got_len[f]) == (0, 0), (f, len(r), ok[f], got_len[f])
        else:
            assert (ok[f], got_len[f]) == (1, len(want)), (f, len(r), ok[f], got_len[f])
            assert bytes(got[f, :len(want)]) == want, f
        verdicts.append(want)
    assert _only_view_written(flat, out, n, max(n_row - 8, 0))
    return verdicts, ok.tolist(), got_len.tolist()


def test_check_is_the_rule(stage):
    c = stage
    rows = _check_rows()
    base = _check_case(c, rows)
    assert sum(v is not None for v in base[0]) >= 38 and sum(v is None for v in base[0]) >= 340   # both verdicts are exercised
    for cap in (1, 3):
        c.set_tuning("grid_cap", cap)
        try:
            again = _check_case(c, rows)
        finally:
            c.set_tuning("grid_cap", 0)
        assert again[1:] == base[1:], cap
    # rows of one length without a length array; lengths beyond the row and below zero are clamped
    rng = np.random.default_rng(5)
    same = [fcs_ref.wrap(bytes(rng.integers(0, 256, 100, dtype=np.uint8))) + bytes(5) for _ in range(9)]
    same[3] = same[3][:50] + bytes([same[3][50] ^ 1]) + same[3][51:]
    v = _check_case(c, same, use_lens=False)[0]
    assert [x is not None for x in v] == [True, True, True, False, True, True, True, True, True]
    n_row = len(same[0])
    mat = np.stack([np.frombuffer(r, np.uint8) for r in same[:3]])
    got, got_len, ok = c.fcs_check(c.to_device(mat), torch.tensor([n_row + 7, -1, n_row], dtype=torch.int32))
    c.synchronize()
    assert ok.tolist() == [1, 0, 1] and got_len.tolist() == [100, 0, 100]


# ---------------------------------------------------------------------------------------------------------- 3. argument checks
def test_stage_argument_checks(stage):
    c = stage
    wrap, check = c.lib.ofdm_fcs_wrap_batch, c.lib.ofdm_fcs_check_batch
    buf = torch.full((4096,), 0x5A, dtype=torch.uint8, device=c.device)
    i32 = torch.zeros((8,), dtype=torch.int32, device=c.device)
    p = buf.data_ptr()
    assert wrap(c.h, p, 2, 300, None, 300, p + 1024, 308, None) == 0
    assert wrap(c.h, p, 2, 300, None, 300, p + 1024, 308, i32.data_ptr()) == 0
    assert wrap(c.h, p, 2, 299, None, 300, p + 1024, 308, None) == -1          # in_stride < n_bytes
    assert wrap(c.h, p, 2, 300, None, 300, p + 1024, 307, None) == -1          # out_stride < n_bytes + 8
    assert wrap(c.h, p, -1, 300, None, 300, p + 1024, 308, None) == -1
    assert wrap(c.h, p, 2, 300, None, -1, p + 1024, 308, None) == -1
    assert wrap(c.h, None, 2, 300, None, 300, p + 1024, 308, None) == -1
    assert wrap(c.h, p, 2, 300, None, 300, None, 308, None) == -1
    assert wrap(c.h, p, 1, 2 ** 31, None, 2 ** 31 - 8, p + 1024, 2 ** 31 + 8, None) == -2   # n_bytes + 8 > INT32_MAX
    assert check(c.h, p, 2, 308, None, 308, p + 1024, 300, i32.data_ptr(), i32[4:].data_ptr()) == 0
    assert check(c.h, p, 2, 308, None, 308, p + 1024, 300, None, None) == 0
    assert check(c.h, p, 2, 307, None, 308, p + 1024, 300, None, None) == -1   # row_stride < n_row
    assert check(c.h, p, 2, 308, None, 308, p + 1024, 299, None, None) == -1   # out_stride < n_row - 8
    assert check(c.h, p, -1, 308, None, 308, p + 1024, 300, None, None) == -1
    assert check(c.h, p, 2, 308, None, -1, p + 1024, 300, None, None) == -1
    assert check(c.h, None, 2, 308, None, 308, p + 1024, 300, None, None) == -1
    assert check(c.h, p, 2, 308, None, 308, None, 300, None, None) == -1
    assert check(c.h, p, 2, 5, None, 5, None, 0, i32.data_ptr(), i32[4:].data_ptr()) == 0   # rows too short to be valid need no output rows
    c.synchronize()
    assert i32.tolist() == [0, 0, 0, 0, 0, 0, 0, 0]
    # n_frames = 0: OFDM_OK and nothing written
    mark = torch.full((1024,), 0xC3, dtype=torch.uint8, device=c.device)
    assert wrap(c.h, p, 0, 300, None, 300, mark.data_ptr(), 308, None) == 0
    assert check(c.h, p, 0, 308, None, 308, mark.data_ptr(), 300, None, None) == 0
    c.synchronize()
    assert bool((mark == 0xC3).all())


# ---------------------------------------------------------------------------------------------------------- 3b. the other reduction
# the same tests, unchanged, on the bit-serial kernels k_fcs_wrap<true> / k_fcs_check<true>: zlib.crc32 is the reference of both
@pytest.mark.parametrize("n_bytes", WRAP_SIZES)
def test_wrap_is_zlib_bitserial(bitserial, n_bytes):
    test_wrap_is_zlib(bitserial, n_bytes)


@pytest.mark.parametrize("test", [test_wrap_long_rows, test_wrap_many_rows_per_wavefront, test_check_is_the_rule, test_stage_argument_checks],
                         ids=lambda t: t.__name__[5:])
def test_stage_bitserial(bitserial, test):
    test(bitserial)


# ---------------------------------------------------------------------------------------------------------- 4 + 5. the frame modes
MODE_CASES = [(64, m) for m in fcs_ref.BASE_MODES] + [(n, m) for n in (256, 1024) for m in (0, 1, 12, 32)]


@functools.lru_cache(maxsize=None)
def _mode_case(n_fft, mode):
    """5 ragged payload rows, their envelopes, and the frames of both contexts"""
    c, base = _ctx(FCS + mode, n_fft), _ctx(mode, n_fft)
    n = 100 if n_fft == 64 else 700
    rng = np.random.default_rng(17 * n_fft + mode)
    pay = rng.integers(0, 256, (5, n), dtype=np.uint8)
    lens = np.array([0, 1, n // 2, n, n], np.int32)
    env = np.zeros((5, n + 8), np.uint8)
    for f in range(5):
        e = fcs_ref.wrap(bytes(pay[f, :lens[f]]))
        env[f, :len(e)] = np.frombuffer(e, np.uint8)
    return c, base, n, pay, lens, env


@pytest.mark.parametrize("n_fft,mode", MODE_CASES)
def test_transmit_is_the_base_frame_of_the_envelope(n_fft, mode):
    c, base, n, pay, lens, env = _mode_case(n_fft, mode)
    for q in (0, 1, n, 560):
        assert c.coded_len(q) == base.coded_len(q + 8), (mode, q)
        assert c.data_symbols(q) == base.data_symbols(q + 8), (mode, q)
        assert c.frame_samples(q) == base.frame_samples(q + 8) == (10 + c.data_symbols(q)) * c.S, (mode, q)
    got = c.encode_batch(c.to_device(pay), lens=torch.from_numpy(lens))
    assert c.last_dispatch().split("+")[0] == "k_fcs_wrap", c.last_dispatch()
    want = base.encode_batch(base.to_device(env), lens=torch.from_numpy(lens + 8))
    assert "k_fcs_wrap" not in base.last_dispatch()
    c.synchronize(); base.synchronize()
    assert got.shape == want.shape and torch.equal(got, want), (n_fft, mode)
    full = np.stack([np.frombuffer(fcs_ref.wrap(bytes(pay[f])), np.uint8) for f in range(5)])
    got = c.encode_batch(c.to_device(pay))
    want = base.encode_batch(base.to_device(full))
    c.synchronize(); base.synchronize()
    assert torch.equal(got, want), (n_fft, mode, "lens = None")


def _channel(c, tx, snr, seed):
    """frames this file built itself through the channel of tools/link.py, the delays and CFOs from a fresh generator"""
    return seeded_channel(c, tx, snr, seed, generator(c, seed))


@pytest.mark.parametrize("n_fft,mode", MODE_CASES)
def test_receive_delivers_exactly_the_payload(n_fft, mode):
    c, base, n, pay, lens, env = _mode_case(n_fft, mode)
    tx = c.encode_batch(c.to_device(pay), lens=torch.from_numpy(lens))
    rx = _channel(c, tx, 40.0 + 10.0 * np.log10(n_fft / 64), 40 + n_fft + mode)
    D = c.data_symbols(n)
    r = c.decode_batch(rx, max_symbols=D)
    c.synchronize()
    trace = c.last_dispatch()
    assert trace.split("+")[-1] == "k_fcs_check", trace
    if mode == 0 and n_fft in (64, 1024):
        assert ("k_rxframe%d<finish>" % n_fft) in trace, trace   # the fused frame kernel still runs, finish included
    rb = base.decode_batch(rx, max_symbols=D)
    base.synchronize()
    assert "k_fcs_check" not in base.last_dispatch()
    status, ln, by = r["status"].cpu().numpy(), r["len"].cpu().numpy(), r["bytes"].cpu().numpy()
    bst, bln, bby = rb["status"].cpu().numpy(), rb["len"].cpu().numpy(), rb["bytes"].cpu().numpy()
    for f in range(5):
        p = int(lens[f])
        assert (int(status[f]), int(ln[f])) == (0, p), (n_fft, mode, f, status[f], ln[f])
        assert bytes(by[f, :p]) == bytes(pay[f, :p]), (n_fft, mode, f)
        assert int(bst[f]) == 0 and int(bln[f]) >= p + 8, (n_fft, mode, f, bst[f], bln[f])   # (Hamming and RS deliver padding too)
        assert bytes(bby[f, 4:4 + p]) == bytes(pay[f, :p]) and bytes(bby[f, :p + 8]) == bytes(env[f, :p + 8]), (n_fft, mode, f)
    for k in ("offset", "f_delta", "metric"):
        assert torch.equal(r[k], rb[k]), k


# ---------------------------------------------------------------------------------------------------------- 6. damage is reported
def _decode_with_sentinels(c, rx, D):
    """ofdm_rx_decode_batch into rows at an odd address with 0xEE between them"""
    n = rx.shape[0]
    ob = c.decode_row_bytes(D)
    out, flat = _embed(c, np.zeros((n, ob), np.uint8))
    out.fill_(SENTINEL)
    ln, st = c.empty((n,), torch.int32), c.empty((n,), torch.int32)
    rc = c.lib.ofdm_rx_decode_batch(c.h, rx.data_ptr(), n, rx.shape[1], rx.shape[1], 0, D, out.data_ptr(), ob + 9, ln.data_ptr(), st.data_ptr(),
                                    None, None, None)
    assert rc == 0, rc
    c.synchronize()
    assert _only_view_written(flat, out, n, ob)
    return st.cpu().numpy(), ln.cpu().numpy(), out.cpu().numpy()


@pytest.mark.parametrize("mode", [0, 10])
def test_damage_is_reported_and_neighbours_are_not_touched(mode):
    c, base = _ctx(FCS + mode), _ctx(mode)
    rng = np.random.default_rng(600 + mode)
    p, p_big = 100, 400
    pay = rng.integers(0, 256, (8, p), dtype=np.uint8)
    env = np.stack([np.frombuffer(fcs_ref.wrap(bytes(pay[f])), np.uint8) for f in range(8)]).copy()
    env[1, 4 + 50] ^= 0x01                                       # one byte of the payload
    env[3, 1] ^= 0x01                                            # one byte of the length word: 100 -> 356
    env[5, 4 + p + 2] ^= 0x80                                    # one byte of the check word
    big_pay = rng.integers(0, 256, (1, p_big), dtype=np.uint8)
    big = np.frombuffer(fcs_ref.wrap(bytes(big_pay[0])), np.uint8).reshape(1, -1).copy()
    tx_small = base.encode_batch(base.to_device(env))
    tx_big = base.encode_batch(base.to_device(big))              # a valid frame that max_symbols cuts short
    D = c.data_symbols(p)
    assert D == base.data_symbols(p + 8) < base.data_symbols(p_big + 8)
    tx = torch.zeros((10, tx_big.shape[1]), dtype=torch.complex64, device=c.device)
    tx[:8, :tx_small.shape[1]] = tx_small
    tx[8] = tx_big[0]
    rx = _channel(c, tx, 40.0, 66 + mode)
    g = torch.Generator(device="cuda"); g.manual_seed(4)
    rx[9] = 0.05 * torch.view_as_complex(torch.randn((rx.shape[1], 2), dtype=torch.float32, device=c.device, generator=g))  # noise only
    status, ln, by = _decode_with_sentinels(c, rx, D)
    for f in (0, 2, 4, 6, 7):                                    # the good frames are delivered
        assert (int(status[f]), int(ln[f])) == (0, p) and bytes(by[f, :p]) == bytes(pay[f]), (mode, f, status[f], ln[f])
    for f in (1, 3, 5, 8):
        assert (int(status[f]), int(ln[f])) == (FRAME_FCS, 0), (mode, f, status[f], ln[f])
    assert (int(status[9]), int(ln[9])) == (NOSYNC, 0), (status[9], ln[9])
    # the base context hands the same damage out as good frames
    rb = base.decode_batch(rx, max_symbols=D)
    base.synchronize()
    assert rb["status"].tolist()[:9] == [0] * 9


def test_uncorrectable_rs_block_keeps_its_status():
    api = _api()
    c, inner = _ctx(FCS + 20), _ctx(0)
    rng = np.random.default_rng(84)
    p = 100
    pay = rng.integers(0, 256, (3, p), dtype=np.uint8)
    code = np.stack([np.frombuffer(api.create_transmission_bytes(fcs_ref.wrap(bytes(pay[f]))), np.uint8) for f in range(3)]).copy()
    assert code.shape == (3, 255)
    for i in rng.choice(255, 20, replace=False):                 # beyond 16 byte errors
        code[1, i] ^= int(rng.integers(1, 256))
    for i in rng.choice(255, 9, replace=False):                  # within: corrected, then the check passes
        code[2, i] ^= int(rng.integers(1, 256))
    rx = _channel(c, inner.encode_batch(inner.to_device(code)), 40.0, 84)
    r = c.decode_batch(rx, max_symbols=c.data_symbols(p))
    c.synchronize()
    assert c.last_dispatch().endswith("k_rs255_decode+k_fcs_check"), c.last_dispatch()
    assert r["status"].tolist() == [0, UNCORRECTABLE, 0] and r["len"].tolist() == [p, 0, p]
    for f in (0, 2):
        assert bytes(r["bytes"][f, :p].cpu().numpy()) == bytes(pay[f]), f


# ---------------------------------------------------------------------------------------------------------- 7. wrappers
def test_every_entry_point_in_an_fcs_mode():
    api = _api()
    ecc = FCS + api.ECC_CONV_K7F_R23
    c = _ctx(ecc)
    rng = np.random.default_rng(75)
    p = 200
    pay = rng.integers(0, 256, (6, p), dtype=np.uint8)
    lens = np.array([p, 0, 7, p, 150, p], np.int32)
    tx = c.encode_batch(c.to_device(pay), lens=torch.from_numpy(lens))
    c.synchronize()
    tx_host = c.encode_host(pay, lens=lens, chunk_frames=4)
    assert np.array_equal(tx_host, tx.cpu().numpy())
    rx = _channel(c, tx, 40.0, 75)
    rx[4, 1000:1100] = 0                                         # one frame loses a data symbol behind its length block: reported by every entry point
    D = c.data_symbols(p)
    r, ones = assert_entry_points_agree(api, c, rx, D, dict(ecc=api.ECC_CONV_K7F_R23, fcs=True), chunk_frames=4)
    assert r["status"].tolist() == [0, 0, 0, 0, FRAME_FCS, 0] and r["len"].tolist() == [p, 0, 7, p, 0, p]
    for f, (st, n_out, _, data) in enumerate(ones):         # every entry point agreed with the one-row decode: that is the batch's row
        assert (st, n_out) == (int(r["status"][f]), int(r["len"][f])), f
        assert data == bytes(r["bytes"][f, :n_out].cpu().numpy()) == bytes(pay[f, :n_out]), f
    for f in range(6):                                           # whatever the frame holds, the check is the chain's last kernel
        c.decode_long(rx[f].contiguous(), D)
        assert c.last_dispatch().split("+")[-1] == "k_fcs_check", (f, c.last_dispatch())
    cap = rx[4].contiguous()
    with pytest.raises(api.DecodeError):                         # the damaged frame is an error, not bytes
        api.decode(cap.cpu().numpy(), True, api.QAM64, ecc=api.ECC_CONV_K7F_R23, fcs=True)
    with pytest.raises(api.DecodeError):
        api.decode_long(cap, True, api.QAM64, ecc=api.ECC_CONV_K7F_R23, max_symbols=D, fcs=True)
    # a detection merged from two contexts (each searches its own lag range of one longer capture)
    g = torch.Generator(device="cuda"); g.manual_seed(11)
    long_cap = 0.002 * torch.view_as_complex(torch.randn((40000, 2), dtype=torch.float32, device=c.device, generator=g))
    long_cap[25000:25000 + rx.shape[1]] = rx[3]
    alone = c.decode_long(long_cap, D)
    merged = api.decode_long(long_cap, True, api.QAM64, ecc=api.ECC_CONV_K7F_R23, world=2, max_symbols=D, fcs=True)
    assert (alone["status"], alone["len"]) == (0, p) and (merged["status"], merged["len"], merged["offset"]) == (0, p, alone["offset"])
    assert bytes(merged["bytes"][:p].cpu().numpy()) == bytes(alone["bytes"][:p].cpu().numpy()) == bytes(pay[3])
    # the Hamming and RS modes return exactly what was sent, not their padding
    msg = b"the payload, the whole payload and nothing but the payload"
    for inner in (api.ECC_HAMMING74, api.ECC_RS255_K7F_R34, api.ECC_NONE):
        assert api.decode(api.encode(msg, True, api.QAM16, ecc=inner, fcs=True), True, api.QAM16, ecc=inner, fcs=True) == msg
    # decode_row_bytes is the header's rule: max(R - 8, 0), R = the base mode's row; a row one byte shorter is refused
    body = D * c.bytes_per_symbol - 16
    bits = 8 * (body - 18)                                       # rate 2/3: the largest T with kept(T) <= bits (framed_ref.max_steps)
    T = 2 * (bits // 3) + (1 if bits % 3 == 2 else 0)
    assert c.lib.ofdm_conv_k7_kept_bits(T, 1) <= bits < c.lib.ofdm_conv_k7_kept_bits(T + 1, 1)
    need = T // 8 - 8                                            # the library's rule; the Python rows of a mode without RS hold the whole body
    assert 4 < need <= c.decode_row_bytes(D) == _ctx(api.ECC_CONV_K7F_R23).decode_row_bytes(D) - 8
    for mode, row in ((0, body), (20, 223 * (body // 255 + 1))):
        assert _ctx(FCS + mode).decode_row_bytes(D) == row - 8 and _ctx(mode).decode_row_bytes(D) == row, mode
    assert _ctx(FCS).decode_row_bytes(1) == max(max(_ctx(FCS).bytes_per_symbol - 16, 0) - 8, 4)
    assert assert_refuses_short_rows(c, rx, D, need, accepts=True) == [p, 0]


# ---------------------------------------------------------------------------------------------------------- 8. it earns its keep
# The link test_rs_outer_code_earns_its_keep (tests/test_gpu_rs.py) runs, tools/link.py at N = 64, 64-QAM, guard bands, payload 560, 12 dB, seed 9012.
# Conditions set before the run: rate 3/4 alone hands out at least 8 of 256 frames with status 0 and wrong bytes (that test's
# commentary records 42 failed frames on this link); with the frame check no frame with status 0 differs from what was sent, and at
# least one is reported with OFDM_FRAME_FCS.  Without any code, 64 frames: every frame is wrong with status 0; with the frame check
# every frame is reported.
KEEP_SNR, KEEP_SEED = 12.0, 9012


def _keep(ecc, n_frames):
    c = _ctx(ecc)
    pay, rx = link_on(c, n_frames, 560, KEEP_SNR, KEEP_SEED)
    r = c.decode_batch(rx, max_symbols=c.data_symbols(560))
    c.synchronize()
    right, ok = delivered(r, pay, 560)
    return int(right.sum()), int((ok & ~right).sum()), int((r["status"] == FRAME_FCS).sum()), int((~ok).sum())


def test_frame_check_earns_its_keep():
    api = _api()
    right, wrong, _, reported = _keep(api.ECC_CONV_K7F_R34, 256)
    print(f"rate 3/4 alone: {right} right, {wrong} wrong with status 0, {reported} reported of 256")
    assert wrong >= 8, wrong                                     # the hole is there
    right_f, wrong_f, fcs_f, reported_f = _keep(FCS + api.ECC_CONV_K7F_R34, 256)
    print(f"frame check + rate 3/4: {right_f} right, {wrong_f} wrong with status 0, {reported_f} reported ({fcs_f} by the check) of 256")
    assert wrong_f == 0, wrong_f
    assert fcs_f >= 1, fcs_f
    assert right_f + reported_f == 256
    right, wrong, _, reported = _keep(api.ECC_NONE, 64)
    print(f"no code: {right} right, {wrong} wrong with status 0, {reported} reported of 64")
    assert (right, wrong) == (0, 64), (right, wrong, reported)
    right_f, wrong_f, fcs_f, reported_f = _keep(FCS + api.ECC_NONE, 64)
    print(f"frame check alone: {right_f} right, {wrong_f} wrong with status 0, {reported_f} reported ({fcs_f} by the check) of 64")
    assert (right_f, wrong_f, reported_f) == (0, 0, 64), (right_f, wrong_f, reported_f)
